"""Regenerate tests/golden/ref_group_kmers.npz: the AA 12-mers the reference's OWN extraction code emits
for the grouping workflow (kmerFormat 3: KmerScanner_dna2aa(12); kmerFormat 5: SyncmerScanner_dna2aa(12, s),
groupGeneration.cpp:65-69), in emission order.

Runs only where the reference tree is mounted; the committed .npz is what the tests read. Nothing of
the reference enters the repository: as in make_ref_scanners.py the code is cut out of the
reference's files at run time, compiled in a temporary directory, run and deleted. The cut code:
* `class KmerScanner`, `class KmerScanner_dna2aa` (KmerScanner.h:11-47, 185-261) and
  `class SyncmerScanner_dna2aa` (SyncmerScanner.h:192-295), whole, as written
* the `atcg` / `iRCT` tables, `LocalUtil::getMaxCoveredLength`, `KmerExtractor::fillQueryKmerBuffer`
with make_ref_scanners.py's minimal declarations and its fillQueryKmerBuffer driver (mate 2 under
mate 1's seqID). Reads: the 112 reads of ref_scanners.npz, plus reads with an N every 11, 12 and 13
codons (valid stretches of 10, 11 and 12 codons: none, none and exactly one 12-mer window in frame 0).
Reads whose mates cannot hold a 12-mer are single-end only, so the shared empty-read rule does not bear.
"""
import pathlib
import re
import subprocess
import tempfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REF = pathlib.Path("/root/reference/src/commons")

from make_ref_functions import definitions  # noqa: E402
from make_ref_scanners import class_text  # noqa: E402


def program() -> str:
    ks = (REF / "KmerScanner.h").read_text()
    ss = (REF / "SyncmerScanner.h").read_text()
    cc = (REF / "common.cpp").read_text()
    lu = (REF / "LocalUtil.h").read_text()
    ke = (REF / "KmerExtractor.cpp").read_text()
    classes = [class_text(ks, "class KmerScanner {"), class_text(ks, "class KmerScanner_dna2aa : public KmerScanner {"),
               class_text(ss, "class SyncmerScanner_dna2aa : public KmerScanner_dna2aa {")]
    tables = [cc[m.start():cc.index(";", m.start()) + 1] for m in re.finditer(r"const std::string (atcg|iRCT) =", cc)]
    assert len(tables) == 2
    covered = definitions(lu, r"template\s*<typename T>\s*T LocalUtil::getMaxCoveredLength\(")
    fill = definitions(ke, r"void KmerExtractor::fillQueryKmerBuffer\(")
    assert len(covered) == 1 and len(fill) == 1
    return "\n".join([
        "#include <cstdint>", "#include <cstdio>", "#include <cstdlib>", "#include <deque>", "#include <iostream>",
        "#include <string>", "#include <vector>", '#include "GeneticCode.h"',
        "typedef int TaxID;",
        "struct Kmer {",
        "  uint64_t value; uint32_t pos; uint32_t seqID; uint8_t frame;",
        "  Kmer() : value(0), pos(0), seqID(0), frame(0) {}",
        "  Kmer(uint64_t v, TaxID t) : value(v), pos((uint32_t)t), seqID(0), frame(0) {}",
        "  Kmer(uint64_t v, uint32_t p) : value(v), pos(p), seqID(0), frame(0) {}",
        "  Kmer(uint64_t v, uint32_t s, uint32_t p, uint8_t f) : value(v), pos(p), seqID(s), frame(f) {}",
        "};",
        *tables, *classes,
        "struct LocalUtil { template<typename T> static T getMaxCoveredLength(T queryLength); };", *covered,
        "template <typename T> struct Buffer { T *buffer; };",
        "struct KmerExtractor {",
        "  KmerScanner **kmerScanners;",
        "  void fillQueryKmerBuffer(const char *seq, int seqLen, Buffer<Kmer> &kmerBuffer, size_t &posToWrite,"
        " uint32_t seqID, uint32_t offset);",
        "};", *fill, DRIVER])


# stdin: "<syncmer> <smerLen> <nReads>", then per read "<len1> <len2>" and the mates' bases on their own
# lines (len2 = 0: single-end). stdout: per emitted k-mer "value seqID frame".
DRIVER = r"""
int main() {
  int syncmer, smerLen; long n;
  if (scanf("%d %d %ld", &syncmer, &smerLen, &n) != 3) return 1;
  GeneticCode gc(false);
  KmerScanner *sc = syncmer ? (KmerScanner *)new SyncmerScanner_dna2aa(gc, 12, smerLen)
                            : (KmerScanner *)new KmerScanner_dna2aa(gc, 12);
  KmerExtractor ex; ex.kmerScanners = &sc;
  std::vector<Kmer> buf(1 << 22);
  Buffer<Kmer> kb{buf.data()};
  static char s1[1 << 20], s2[1 << 20];
  for (long i = 0; i < n; i++) {
    int l1, l2;
    if (scanf("%d %d", &l1, &l2) != 2) return 2;
    if (scanf("%s", s1) != 1) return 3;
    if (l2 && scanf("%s", s2) != 1) return 4;
    size_t pos = 0;
    ex.fillQueryKmerBuffer(s1, l1, kb, pos, (uint32_t)i + 1, 0);
    if (l2) ex.fillQueryKmerBuffer(s2, l2, kb, pos, (uint32_t)i + 1, (uint32_t)LocalUtil::getMaxCoveredLength(l1) + 3);
    for (size_t k = 0; k < pos; k++)
      printf("%llu %u %u\n", (unsigned long long)buf[k].value, buf[k].seqID, (unsigned)buf[k].frame);
  }
  return 0;
}
"""

CONFIGS = [("fmt3", 0, 5), ("fmt5_s5", 1, 5), ("fmt5_s6", 1, 6)]


def n_reads(rng):
    """Reads with an N every `period` codons of frame 0 (at a random base of that codon)."""
    alpha = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for period in (11, 12, 13):
        for codons, extra in ((80, 0), (67, 1), (53, 2)):
            s = alpha[rng.integers(0, 4, 3 * codons + extra)].copy()
            for c in range(period - 1, codons, period):
                s[3 * c + int(rng.integers(0, 3))] = ord("N")
            out.append(s.tobytes().decode())
    return [(a, "") for a in out] + [(out[0], out[7]), (out[8], out[2])]


if __name__ == "__main__":
    base = np.load(HERE / "ref_scanners.npz")
    rs = list(zip(base["seq1"].tolist(), base["seq2"].tolist())) + n_reads(np.random.default_rng(20261020))
    arrays = {"seq1": np.array([a for a, _ in rs]), "seq2": np.array([b for _, b in rs])}
    with tempfile.TemporaryDirectory() as d:
        src = pathlib.Path(d) / "ref_group_kmers.cpp"
        exe = pathlib.Path(d) / "ref_group_kmers"
        src.write_text(program())
        subprocess.run(["g++", "-O1", "-std=c++17", f"-I{REF}", str(src), "-o", str(exe)], check=True)
        for name, syn, smer in CONFIGS:
            inp = [f"{syn} {smer} {len(rs)}"]
            for a, b in rs:
                inp.append(f"{len(a)} {len(b)}")
                inp.append(a)
                if b:
                    inp.append(b)
            got = subprocess.run([str(exe)], input="\n".join(inp) + "\n", capture_output=True, text=True,
                                 check=True).stdout.split()
            v = np.array(got, dtype=np.uint64).reshape(-1, 3)
            arrays[f"{name}_value"] = v[:, 0]
            arrays[f"{name}_seq"] = v[:, 1].astype(np.uint32)
            arrays[f"{name}_frame"] = v[:, 2].astype(np.uint8)
            print(name, len(v), "k-mers;", int(np.isin(v[:, 1], np.arange(113, len(rs) + 1)).sum()), "from the N reads")
    np.savez_compressed(HERE / "ref_group_kmers.npz", **arrays)
    print("wrote", HERE / "ref_group_kmers.npz", (HERE / "ref_group_kmers.npz").stat().st_size, "bytes")
