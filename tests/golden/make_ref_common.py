"""Regenerate tests/golden/ref_common.npz: what the reference's OWN code gives for the common-k-mer DB
(create_common_kmer_list): the AA 12-mers KmerExtractor::extractKmer_dna2aa emits for designed genomes, and the
diffIdx / info / split files IndexCreator::mergeTargetFiles<COMMON_KMER> writes for designed sets of flush files.

Runs only where the reference tree is mounted; the committed .npz is what the tests read. Nothing of the
reference enters the repository: as in make_ref_merge.py and make_ref_group_kmers.py the code is cut out of the
reference's files at run time into throw-away C++ files in a temporary directory, compiled, run and deleted.

Two programs:
* extraction: make_ref_group_kmers.py's cut (`class KmerScanner`, `KmerScanner_dna2aa`, `SyncmerScanner_dna2aa`,
  the `atcg` / `iRCT` tables) with `KmerExtractor::extractKmer_dna2aa` (KmerExtractor.cpp:388-418) in place of
  fillQueryKmerBuffer, whole, as written; a stand-in Kmer that keeps (value, taxID, species).
* merge: make_ref_merge.py's program, unchanged but for two textual replacements, each of which must hit
  exactly once (asserted): the stand-in IndexCreator's `kmerFormat = 2` becomes 3 (AminoAcidPart is then the
  whole value, IndexCreator.h:209-214) and the driver's `mergeTargetFiles<FilterMode::DB_CREATION>` becomes
  `<FilterMode::COMMON_KMER>`. Everything make_ref_merge.py says about the buffer-size literals, the one-pass
  and many-pass settings and the stand-ins holds here.
Both are also built with -fsanitize=address,undefined -fno-sanitize-recover=all (stand-alone programs with
their own main) and run over every genome configuration / every case's one-pass setting with 1 and 16 threads;
they must exit clean with the same output (leak reports off: mergeTargetFiles never frees its readers).

Flush files. A flush file of createCommonKmerIndex is what filterKmers<DB_CREATION> leaves of one batch: one
entry per (value, species), its taxID the LCA of the group's taxIDs. The designed files here are (value, taxID)
lists finished by make_ref_merge.finish and encoded by tests/group_filter_cases.encode_diffidx (the plain-Python
encoder ref_group_filter.npz pins), as make_ref_merge.py's inputs are. The taxonomy hangs every strain directly
under its species, so a file's taxID always has its species in taxId2speciesId (a per-flush LCA between a strain
and its species would map to species 0, IndexCreator.cpp:680-689; deeper trees are held to tests/common_expect.py
only).

The expectation is the one-pass answer (value buffers larger than every input). COMMON_KMER inputs repeat values
inside a file by construction, so the many-pass setting may end an outer pass inside a run of equal values
(DeltaIdxReader::getValues, see make_ref_merge.py); per case `many_agree` records whether the many-pass runs gave
the same bytes, and nothing is drawn again. The three thread counts must agree within a setting (asserted).

The one-flush quirk (IndexCreator.cpp:296-299: with numOfFlush == 1 createCommonKmerIndex returns before the
COMMON_KMER merge, so its single flush file IS the "common" DB) is recorded once, as `one_flush_*`: the single
file (what the reference would leave: every (value, species) k-mer) next to what the COMMON_KMER rule gives over
that same file. It is not an expectation of any test of the device, which always applies the rule.

`from_genomes`: the flush files of the fixture's own genomes (format 3), three flushes that split the genomes by
species (no (value, species) pair in two files, so numOfKmerBeforeMerge equals the distinct pairs), each made by
tests/merge_expect.expected_merge (filterKmers<DB_CREATION> as ref_merge.npz pins it).
"""
import os
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

import make_ref_merge as mrm  # noqa: E402
from dbref import Tree, decode_diff, diff_words  # noqa: E402
from group_filter_cases import encode_diffidx  # noqa: E402
from make_ref_functions import definitions  # noqa: E402
from make_ref_scanners import class_text  # noqa: E402
from metabuli_work_amd import synth  # noqa: E402
from tests.merge_expect import expected_merge  # noqa: E402

THREADS = mrm.THREADS
TAXONOMY = dict(n_species=12, strains_per_species=3, seed=5, n_genera=8)  # one genus under Eukaryota: LCA(all) = root
SEED = 20261021
CONFIGS = [("fmt3", 0, 5), ("fmt5_s5", 1, 5), ("fmt5_s6", 1, 6)]
TOP = (1 << 60) - 1  # the largest AA 12-mer value


# ---- the programs -------------------------------------------------------------------------------------------
def merge_program() -> str:
    text = mrm.program()
    for old, new in (("int kmerFormat = 2;", "int kmerFormat = 3;"),
                     ("mergeTargetFiles<FilterMode::DB_CREATION>()", "mergeTargetFiles<FilterMode::COMMON_KMER>()")):
        assert text.count(old) == 1, f"{old!r}: {text.count(old)} hits"
        text = text.replace(old, new)
    return text


def extract_program() -> str:
    ks = (REF / "KmerScanner.h").read_text()
    ss = (REF / "SyncmerScanner.h").read_text()
    cc = (REF / "common.cpp").read_text()
    ke = (REF / "KmerExtractor.cpp").read_text()
    classes = [class_text(ks, "class KmerScanner {"), class_text(ks, "class KmerScanner_dna2aa : public KmerScanner {"),
               class_text(ss, "class SyncmerScanner_dna2aa : public KmerScanner_dna2aa {")]
    tables = [cc[m.start():cc.index(";", m.start()) + 1] for m in re.finditer(r"const std::string (atcg|iRCT) =", cc)]
    assert len(tables) == 2
    ext = definitions(ke, r"void KmerExtractor::extractKmer_dna2aa\(")
    assert len(ext) == 1
    return "\n".join([
        "#include <cstdint>", "#include <cstdio>", "#include <cstdlib>", "#include <deque>", "#include <iostream>",
        "#include <string>", "#include <vector>", '#include "GeneticCode.h"',
        "typedef int TaxID;",
        "struct Kmer {",
        "  uint64_t value; uint32_t pos; TaxID taxId; TaxID speciesId;",
        "  Kmer() : value(0), pos(0), taxId(0), speciesId(0) {}",
        "  Kmer(uint64_t v, uint32_t p) : value(v), pos(p), taxId(0), speciesId(0) {}",
        "  Kmer(uint64_t v, TaxID t, TaxID s) : value(v), pos(0), taxId(t), speciesId(s) {}",
        "};",
        *tables, *classes,
        "template <typename T> struct Buffer { T *buffer; };",
        "struct KmerExtractor {",
        "  KmerScanner **kmerScanners;",
        "  void extractKmer_dna2aa(const char *seq, int seqLen, Buffer<Kmer> &kmerBuffer, size_t &posToWrite,"
        " uint32_t seqId1, uint32_t seqId2);",
        "};", *ext, EXTRACT_DRIVER])


# stdin: "<syncmer> <smerLen> <nGenomes>", then per genome "<len> <taxID> <species>" and its bases on a line of
# their own. stdout: per emitted k-mer "value genome taxID species".
EXTRACT_DRIVER = r"""
int main() {
  int syncmer, smerLen; long n;
  if (scanf("%d %d %ld", &syncmer, &smerLen, &n) != 3) return 1;
  GeneticCode gc(false);
  KmerScanner *sc = syncmer ? (KmerScanner *)new SyncmerScanner_dna2aa(gc, 12, smerLen)
                            : (KmerScanner *)new KmerScanner_dna2aa(gc, 12);
  KmerExtractor ex; ex.kmerScanners = &sc;
  std::vector<Kmer> buf(1 << 20);
  Buffer<Kmer> kb{buf.data()};
  std::vector<char> s(1 << 20);
  for (long i = 0; i < n; i++) {
    int len, tax, sp;
    if (scanf("%d %d %d", &len, &tax, &sp) != 3) return 2;
    if (len >= (int)s.size() || 6 * (size_t)len >= buf.size()) return 5;
    if (scanf("%s", s.data()) != 1) return 3;
    size_t pos = 0;
    ex.extractKmer_dna2aa(s.data(), len, kb, pos, (uint32_t)tax, (uint32_t)sp);
    for (size_t k = 0; k < pos; k++)
      printf("%llu %ld %d %d\n", (unsigned long long)buf[k].value, i, buf[k].taxId, buf[k].speciesId);
  }
  delete sc;
  return 0;
}
"""


# ---- the world ----------------------------------------------------------------------------------------------
class World(mrm.World):
    def __init__(self):
        self.taxo = synth.make_taxonomy(**TAXONOMY)
        self.tree = Tree(self.taxo)
        leaves = [t for t, r in zip(self.taxo.taxid.tolist(), self.taxo.rank) if r == "no rank" and t != 1]
        self.species = sorted({int(self.tree.sp[t]) for t in leaves})
        self.strains = {s: sorted(t for t in leaves if self.tree.sp[t] == s) for s in self.species}
        self.leaves = np.array(leaves, np.int64)
        assert 0 not in self.species and len(self.species) == TAXONOMY["n_species"]
        # every strain hangs directly under its species
        par = dict(zip(self.taxo.taxid.tolist(), self.taxo.parent.tolist()))
        assert all(par[t] == int(self.tree.sp[t]) for t in leaves)
        self.genus = {s: par[s] for s in self.species}
        red = self.species[0]
        for s in self.species[1:]:
            red = self.tree.lca(red, s)
        assert red == 1 and len(set(self.genus.values())) >= 3


def genomes(w, rng):
    """Short genomes with planted shared segments, one strain each: lengths 35 .. 39 (the first window of each
    frame appears and disappears), N, IUPAC and lower-case letters, a stop-codon run."""
    alpha = np.frombuffer(b"ACGT", np.uint8)

    def dna(n):
        return alpha[rng.integers(0, 4, n)].tobytes().decode()

    seg_sp = dna(120)      # strains of one species only
    seg_genus = dna(120)   # two species of one genus
    seg_two = dna(120)     # species of two genera
    seg_all = dna(90)      # every species
    by_genus = {}
    for s in w.species:
        by_genus.setdefault(w.genus[s], []).append(s)
    pair = next(v for v in by_genus.values() if len(v) >= 2)[:2]
    other = next(s for s in w.species if w.genus[s] != w.genus[pair[0]])
    out = []
    for i, s in enumerate(w.species):
        for k, t in enumerate(w.strains[s][:2]):
            g = dna(150 + 7 * i + k)
            if s == w.species[0]:
                g += seg_sp
            if s in pair:
                g += seg_genus + dna(5 + k)
            if s in (pair[0], other):
                g += dna(1 + k) + seg_two
            g += dna(k) + seg_all + dna(31 + i)
            out.append((g, t))
    t0 = w.strains[w.species[3]][2]
    for n in (35, 36, 37, 38, 39):
        out.append((seg_all[:n], t0))
    out.append((dna(60) + "N" + dna(50) + "RYKM" + dna(47) + dna(60).lower() + "TAATAGTGATAA" * 4 + dna(40), t0))
    return out


# ---- the designed flush files -------------------------------------------------------------------------------
def aa_values(rng, n):
    """n distinct 60-bit values above 0 and below TOP, some close together (one-word deltas)."""
    base = np.unique(rng.integers(1, TOP, n, dtype=np.uint64))
    near = base[: n // 4] + rng.integers(1, 1 << 14, len(base[: n // 4]), dtype=np.uint64)
    out = np.unique(np.concatenate([base, near]))
    out = out[(out > 1) & (out < TOP)]
    return rng.permutation(out)[:n]


def designed(n_files, split_num, first_kept, last_kept, n=240):
    def build(w, rng):
        v = aa_values(rng, n)
        files = [[] for _ in range(n_files)]
        sp = w.species
        by_genus = {}
        for s in sp:
            by_genus.setdefault(w.genus[s], []).append(s)
        sister = next(x for x in by_genus.values() if len(x) >= 2)
        far = [sister[0], next(s for s in sp if w.genus[s] != w.genus[sister[0]])]

        def strain(s):
            return int(rng.choice(w.strains[s]))

        for j, x in enumerate(v.tolist()):
            # of 16 values 13 are kept and about 36 entries written, so that even splitNum 4 (sizeOfSplit a third
            # of the entries) reaches its offsets among the kept values
            kind = {0: 0, 1: 1, 4: 4 if j % 48 == 4 else 3, 5: 5, 6: 6, 7: 7}.get(j % 16, 2 + j % 2)
            f = int(rng.integers(0, n_files))
            g = (f + 1 + int(rng.integers(0, n_files - 1))) % n_files
            s = sp[int(rng.integers(0, len(sp)))]
            if kind == 0:      # one species, one file
                files[f].append((x, strain(s)))
            elif kind == 1:    # one species in several files (two strains, or the same taxID): dropped
                for q in range(min(n_files, 3)):
                    files[(f + q) % n_files].append((x, w.strains[s][q % len(w.strains[s])]))
            elif kind == 2:    # two species inside one file
                files[f] += [(x, strain(sister[0])), (x, strain(sister[1]))]
            elif kind == 3:    # two species, only across files
                files[f].append((x, strain(far[0])))
                files[g].append((x, strain(far[1])))
            elif kind == 4:    # every species (LCA = root), spread over the files
                for q, s2 in enumerate(sp):
                    files[q % n_files].append((x, strain(s2)))
            elif kind == 5:    # two species of one genus across files, one of them twice (two strains)
                files[f] += [(x, w.strains[sister[0]][0]), (x, w.strains[sister[0]][1])]
                files[g].append((x, strain(sister[1])))
            elif kind == 6:    # three species of two genera in three entries of one or two files
                files[f] += [(x, strain(sister[0])), (x, strain(far[1]))]
                files[g].append((x, strain(sister[1])))
            else:              # the same taxID in two files: dropped
                files[f].append((x, w.strains[s][0]))
                files[g].append((x, w.strains[s][0]))
        # the smallest and the largest value of all, kept (two species across files) or dropped (one species twice)
        for x, kept in ((1, first_kept), (TOP, last_kept)):
            files[0].append((x, strain(far[0])))
            files[n_files - 1].append((x, strain(far[1] if kept else far[0])))
        return files, split_num
    return build


def cases():
    out = []
    for n_files, split_num, fk, lk in ((2, 4, True, False), (2, 16, False, True), (3, 16, True, True), (3, 4096, False, False),
                                        (8, 4, False, True), (8, 16, True, False), (8, 4096, True, True)):
        out.append((f"in{n_files}_s{split_num}_{'k' if fk else 'd'}{'k' if lk else 'd'}", designed(n_files, split_num, fk, lk)))
    return out


def write_inputs(d, inputs):
    for i, (v, t) in enumerate(inputs):
        words = encode_diffidx(v)
        assert np.array_equal(decode_diff(words), v) and len(words) == int(diff_words(v).sum())
        words.tofile(pathlib.Path(d) / f"in{i}.diffIdx")
        t.astype(np.uint32).tofile(pathlib.Path(d) / f"in{i}.info")


def reference_case(exe, san, d, tax, inputs, split_num, name):
    """(one-pass result, many-pass runs agree with it) of one case; the thread counts must agree in a setting."""
    assert all(len(v) for v, _ in inputs) and sum(len(v) for v, _ in inputs) >= 2
    write_inputs(d, inputs)
    sizes = mrm.one_pass_sizes(inputs)
    one = [mrm.run_ref(exe, d, tax, inputs, split_num, th, sizes) for th in THREADS]
    assert all(r[3] == 1 for r in one), f"{name}: the one-pass setting took {[r[3] for r in one]} passes"
    assert all(mrm.same(one[0], r) for r in one), f"{name}: the one-pass runs differ between thread counts"
    for th in (1, 16):
        assert mrm.same(one[0], mrm.run_ref(san, d, tax, inputs, split_num, th, sizes)), f"{name}: sanitizer build differs"
    many = [mrm.run_ref(exe, d, tax, inputs, split_num, th, mrm.MANY) for th in THREADS]
    agree = all(mrm.same(one[0], r) for r in many)
    return one[0], agree


def store(out, name, inputs, split_num, result, agree):
    out[f"{name}_n_in"] = np.int64(len(inputs))
    out[f"{name}_split_num"] = np.int64(split_num)
    out[f"{name}_many_agree"] = np.int64(agree)
    for i, (v, t) in enumerate(inputs):
        out[f"{name}_in{i}_diffIdx"] = encode_diffidx(v)
        out[f"{name}_in{i}_info"] = t.astype(np.uint32)
    out[f"{name}_diffIdx"], out[f"{name}_info"], out[f"{name}_split"] = result[:3]


def run_extract(exe, gen, syn, smer, w):
    inp = [f"{syn} {smer} {len(gen)}"]
    for g, t in gen:
        inp += [f"{len(g)} {t} {int(w.tree.sp[t])}", g]
    got = subprocess.run([str(exe)], input="\n".join(inp) + "\n", capture_output=True, text=True, check=True).stdout
    return np.array(got.split(), dtype=np.uint64).reshape(-1, 4)


if __name__ == "__main__":
    # mergeTargetFiles never deletes its readers and buffers: the leak report at exit is switched off, every
    # other finding of the sanitizers still ends the run
    os.environ["ASAN_OPTIONS"] = "detect_leaks=0"
    w = World()
    rng = np.random.default_rng(SEED)
    gen = genomes(w, rng)
    out = {"tax_id": w.taxo.taxid, "tax_parent": w.taxo.parent, "tax_rank": np.array(w.taxo.rank),
           "threads": np.array(THREADS), "genomes": np.array([g for g, _ in gen]),
           "genome_taxid": np.array([t for _, t in gen], np.int32)}
    names = []
    with tempfile.TemporaryDirectory() as d:
        d = pathlib.Path(d)
        # extraction
        src = d / "ref_common_extract.cpp"
        src.write_text(extract_program())
        flags = ["-O1", "-std=c++17", "-w", f"-I{REF}", str(src)]
        san_flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.run(["g++", *flags, "-o", str(d / "extract")], check=True)
        subprocess.run(["g++", *san_flags, *flags, "-o", str(d / "extract_san")], check=True)
        for name, syn, smer in CONFIGS:
            v = run_extract(d / "extract", gen, syn, smer, w)
            assert np.array_equal(v, run_extract(d / "extract_san", gen, syn, smer, w)), "sanitizer build differs"
            assert np.array_equal(v[:, 2].astype(np.int64), np.array([gen[int(i)][1] for i in v[:, 1]], np.int64))
            out[f"{name}_value"] = v[:, 0]
            out[f"{name}_genome"] = v[:, 1].astype(np.uint32)
            print(name, len(v), "k-mers of", len(gen), "genomes")
        # merge
        src, exe, san, tax = d / "ref_common.cpp", d / "ref_common", d / "ref_common_san", d / "tax.txt"
        src.write_text(merge_program())
        flags = ["-O1", "-std=c++17", "-fopenmp", "-w", f"-I{REF}", str(src)]
        subprocess.run(["g++", *flags, "-o", str(exe)], check=True)
        subprocess.run(["g++", *san_flags, *flags, "-o", str(san)], check=True)
        w.tax_file(tax)
        for name, build in cases():
            files, split_num = build(w, np.random.default_rng([SEED, sum(name.encode())]))
            inputs = [mrm.finish(w, f) for f in files]
            res, agree = reference_case(exe, san, d, tax, inputs, split_num, name)
            store(out, name, inputs, split_num, res, agree)
            names.append(name)
            print(f"{name}: {[len(v) for v, _ in inputs]} entries, {len(res[1])} written, "
                  f"{int((res[2].reshape(-1, 3)[1:, 1] != 0).sum())} split entries after entry 0, many-pass agrees: {agree}")
        # the fixture's own genomes as three flushes split by species
        v3, g3 = out["fmt3_value"], out["fmt3_genome"].astype(np.int64)
        tax_of = out["genome_taxid"].astype(np.int64)
        sp_rank = {s: i for i, s in enumerate(w.species)}
        flush_of = np.array([sp_rank[int(w.tree.sp[t])] % 3 for t in tax_of])
        inputs = []
        for f in range(3):
            m = flush_of[g3] == f
            fv, fi = expected_merge(w.tree, [(v3[m], tax_of[g3[m]])])
            inputs.append((fv, fi.astype(np.uint32)))
        res, agree = reference_case(exe, san, d, tax, inputs, 16, "from_genomes")
        store(out, "from_genomes", inputs, 16, res, agree)
        out["from_genomes_flush"] = flush_of.astype(np.int32)
        names.append("from_genomes")
        print(f"from_genomes: {[len(v) for v, _ in inputs]} entries, {len(res[1])} written, many-pass agrees: {agree}")
        # the one-flush quirk: the single flush file is what the reference leaves; the rule gives less
        m = np.isin(tax_of[g3], [t for t in tax_of if sp_rank[int(w.tree.sp[t])] < 4])
        fv, fi = expected_merge(w.tree, [(v3[m], tax_of[g3[m]])])
        one = [(fv, fi.astype(np.uint32))]
        res, agree = reference_case(exe, san, d, tax, one, 16, "one_flush")
        store(out, "one_flush", one, 16, res, agree)
        print(f"one_flush: the single flush file holds {len(fv)} k-mers (what numOfFlush == 1 leaves as the DB), "
              f"the COMMON_KMER rule over it keeps {len(res[1])}")
    out["cases"] = np.array(names)
    np.savez_compressed(HERE / "ref_common.npz", **out)
    print("wrote", HERE / "ref_common.npz", (HERE / "ref_common.npz").stat().st_size, "bytes")
