"""Regenerate tests/golden/ref_assign.npz: what the reference's OWN per-read scoring code returns for
fixed match lists (round 8). Until now getMatchPaths, getBestSpeciesMatches, chooseBestTaxon,
filterRedundantMatches, lowerRankClassification / getSpeciesCladeCounts / BFS and compareDna were
restatement-only on both sides (oracle/orc_taxonomer.cpp, orc_match.cpp and the K5 / K6 kernels).

Fixture-time only, never imported by a test. As in make_ref_paths.py the code is cut out of
/root/reference/src/commons at run time into a throw-away C++ file in a temporary directory next to
stand-in declarations, compiled with BitManipulateMacros.h in place (g++ -O1 -std=c++17
-ffp-contract=off), run and deleted. The same program is also built with -fsanitize=address,undefined
and fed every case; it must exit clean with the same output (the inputs keep the reference inside
defined behaviour: filterRedundantMatches indexes by pos / dnaShift without a bound check).

The cut code (reference file:line):
* Taxonomer.h:15-23 `struct TaxonScore`, :35-59 `struct MatchPath`, :61-197 `class Taxonomer`
* Taxonomer.cpp:12-85 constructor and destructor, :130-202 chooseBestTaxon, :205-241
  filterRedundantMatches, :252-271 lowerRankClassification, :273-290 getSpeciesCladeCounts, :292-314
  BFS, :316-408 getBestSpeciesMatches, :410-485 combineMatchPaths / isMatchPathOverlapped /
  trimMatchPath, :487-648 getMatchPaths, :650-699 calScoreIncrement / calHammingDistIncrement /
  isConsecutive x2 / isConsecutive2 x2, :701-713 ensureArraySize
* Match.h:32-86 Match's score methods; common.h:95-128 `struct Query`
* KmerMatcher.cpp:1117-1146 compareDna, :1149-1166 compareMatches (std::sort on it orders each
  DB's matches); KmerMatcher.h:66-158 the Hamming tables, :348-360 getHammingDistanceSum, :386-416
  getHammings / getHammings_reverse

Stand-ins (declarations only): QueryKmerInfo / Match with the fields the cut code reads, a
LocalParameters with the fields it reads, `TaxonCounts` (MMseqs2's NcbiTaxonomy.h, not in the
reference tree: two counters and a child list), a KmerMatcher holding kmerFormat and the cut tables.
The one place with logic of our own is `TaxonomyWrapper` over a parent table: taxonNode, getString,
getTaxIdAtRank, LCA(a, b), LCA(vector), IsAncestor, getEukaryotaTaxID as plain parent walks. These
are MMseqs2 services and stay "parity unpinned"; the inputs stay away from their edge cases (no
taxID 0, no ID outside the tree, every targetId under its speciesId, getTaxIdAtRank only ever asked
for a species' own ID).

The DBs are built exactly as tests/conftest.py:make_db builds them (same DB_CONFIGS row, seeds 11 and
12). Those taxonomies hold no species under Eukaryota (n_genera // 8 == 0) and no node of rank "":
the Eukaryota branch is reached with the Eukaryota node itself as speciesId and targetId
(IsAncestor(x, x) is true), and the rank-"" leaf removal only on `fmt2_acc_blank`, the fmt2_acc
taxonomy with its "no rank" strains' rank strings emptied (see tests/test_ref_assign.py).
One read's taxCnt can hold at most 1 + strains + accessions taxa of one species (7 here). So there is
one more DB, `wide` (tests/ref_assign_fixture.py: 8 genera, so that species sit under Eukaryota, and
one species with 322 strains): Eukaryota species with best depth 4-8 and 9, and reads whose taxCnt
holds 64 / 65 and 256 / 257 distinct taxa (kGroupHash / kTcHash). The tests build that DB themselves.
"""
import pathlib
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parents[1]
REF = pathlib.Path("/root/reference/src/commons")
sys.path.insert(0, str(ROOT))

from make_ref_functions import definitions  # noqa: E402
from make_ref_scanners import class_text  # noqa: E402

DBS = ["fmt2", "fmt1", "fmt2_syncmer", "fmt2_acc"]
# seqMode, accessionLevel (as given on the command line: 0 / 1), minScore, minSpScore, em
PARAM_SETS = [(2, 0, 0.0, 0.0, 0), (3, 1, 0.0, 0.0, 0), (2, 0, 0.15, 0.5, 0), (2, 0, 0.15, 0.0, 1)]
PARAM_COLS = ["seqMode", "accessionLevel", "minConsCnt", "minConsCntEuk", "tieRatioBits", "syncmer", "smerLen",
              "minScoreBits", "minSpScoreBits", "em", "kmerFormat"]


def fbits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


# ---------------------------------------------------------------------------------------------------
# the program
def program() -> str:
    th = (REF / "Taxonomer.h").read_text()
    tx = (REF / "Taxonomer.cpp").read_text()
    mh = (REF / "Match.h").read_text()
    ch = (REF / "common.h").read_text()
    kh = (REF / "KmerMatcher.h").read_text()
    kc = (REF / "KmerMatcher.cpp").read_text()
    m_struct = mh[mh.index("struct Match {"):]
    m_defs = [definitions(m_struct, h)[0] for h in (
        r"float getScore\(", r"virtual float getRightPartScore\(", r"virtual float getLeftPartScore\(",
        r"virtual int getRightPartHammingDist\(", r"virtual int getLeftPartHammingDist\(")]
    heads = [r"Taxonomer::Taxonomer\(", r"Taxonomer::~Taxonomer\(", r"void Taxonomer::chooseBestTaxon\(",
             r"void Taxonomer::filterRedundantMatches\(", r"TaxID Taxonomer::lowerRankClassification\(",
             r"void Taxonomer::getSpeciesCladeCounts\(", r"TaxID Taxonomer::BFS\(",
             r"TaxonScore Taxonomer::getBestSpeciesMatches\(", r"float Taxonomer::combineMatchPaths\(",
             r"bool Taxonomer::isMatchPathOverlapped\(", r"void Taxonomer::trimMatchPath\(",
             r"void Taxonomer::getMatchPaths\(", r"float Taxonomer::calScoreIncrement\(",
             r"int Taxonomer::calHammingDistIncrement\(", r"bool Taxonomer::isConsecutive\(",
             r"bool Taxonomer::isConsecutive2\(", r"void Taxonomer::ensureArraySize\("]
    tax_defs = [d for h in heads for d in definitions(tx, h)]
    assert len(tax_defs) == len(heads) + 2, len(tax_defs)  # isConsecutive{,2}: two overloads each
    tables = kh[kh.index("uint8_t hammingLookup[8][8]"):]
    tables = tables[:tables.index("};", tables.index("HAMMING_LUT7[64]")) + 2]
    km_defs = (definitions(kh, r"(?m)^inline uint8_t KmerMatcher::getHammingDistanceSum\(") +
               definitions(kh, r"(?m)^inline uint16_t KmerMatcher::getHammings\(") +
               definitions(kh, r"(?m)^inline uint16_t KmerMatcher::getHammings_reverse\(") +
               definitions(kc, r"void KmerMatcher::compareDna\(") +
               definitions(kc, r"bool KmerMatcher::compareMatches\("))
    assert len(km_defs) == 5, len(km_defs)
    return "\n".join([
        "#include <algorithm>", "#include <cstdint>", "#include <cstdio>", "#include <cstring>", "#include <iostream>",
        "#include <limits>", "#include <map>", "#include <string>", "#include <unordered_map>",
        "#include <unordered_set>", "#include <vector>", '#include "BitManipulateMacros.h"', "using namespace std;",
        STANDINS_1, "struct Match {",
        "  QueryKmerInfo qInfo; TaxID targetId = 0; TaxID speciesId = 0; uint32_t dnaEncoding = 0;",
        "  uint16_t rightEndHamming = 0; uint8_t hamming = 0;", *m_defs, "};",
        class_text(ch, "struct Query {"), class_text(th, "struct TaxonScore {"), class_text(th, "struct MatchPath {"),
        class_text(th, "class Taxonomer {"), *tax_defs,
        "struct KmerMatcher {", "  int kmerFormat = 2;", tables,
        "  void compareDna(uint64_t query, std::vector<uint64_t> &targetKmersToCompare, std::vector<uint8_t> &hammingDists,"
        " std::vector<size_t> &selectedMatches, std::vector<uint8_t> &selectedHammingSum,"
        " std::vector<uint16_t> &selectedHammings, size_t &selectedMatchIdx, uint8_t frame);",
        "  uint8_t getHammingDistanceSum(uint64_t kmer1, uint64_t kmer2);",
        "  uint16_t getHammings(uint64_t kmer1, uint64_t kmer2);",
        "  uint16_t getHammings_reverse(uint64_t kmer1, uint64_t kmer2);",
        "  static bool compareMatches(const Match &a, const Match &b);", "};", *km_defs, DRIVER])


# Declarations only, except TaxonomyWrapper: plain parent walks (MMseqs2 services, parity unpinned).
STANDINS_1 = r"""
typedef int TaxID;
struct QueryKmerInfo { uint32_t pos = 0; uint32_t sequenceID = 0; uint8_t frame = 0; };
struct LocalParameters {
  int maxGap = 0, accessionLevel = 0, minSSMatch = 0, minConsCnt = 4, minConsCntEuk = 9;
  float tieRatio = 0.95f;
  int syncmer = 0, smerLen = 5, seqMode = 2, reducedAA = 0;
  float minScore = 0.f, minSpScore = 0.f;
  bool em = false;
  int printLog = 0;
};
struct TaxonNode { TaxID taxId; TaxID parentTaxId; size_t rankIdx; };
struct TaxonCounts { unsigned int taxCount = 0; unsigned int cladeCount = 0; std::vector<TaxID> children; };
struct TaxonomyWrapper {
  std::vector<TaxonNode> nodes; std::vector<int> row; std::vector<std::string> ranks; TaxID euk = 0;
  const TaxonNode *taxonNode(TaxID t) const { return &nodes.at(row.at(t)); }
  const char *getString(size_t i) const { return ranks.at(i).c_str(); }
  TaxID getEukaryotaTaxID() const { return euk; }
  TaxID getOriginalTaxID(TaxID t) const { return t; }
  bool IsAncestor(TaxID ancestor, TaxID child) const {
    for (TaxID t = child;; t = taxonNode(t)->parentTaxId) {
      if (t == ancestor) return true;
      if (taxonNode(t)->parentTaxId == t) return false;
    }
  }
  TaxID LCA(TaxID a, TaxID b) const {
    for (TaxID t = a;; t = taxonNode(t)->parentTaxId) {
      if (IsAncestor(t, b)) return t;
      if (taxonNode(t)->parentTaxId == t) return t;
    }
  }
  const TaxonNode *LCA(const std::vector<TaxID> &v) const {
    TaxID r = v.at(0);
    for (size_t i = 1; i < v.size(); i++) r = LCA(r, v[i]);
    return taxonNode(r);
  }
  TaxID getTaxIdAtRank(TaxID t, const std::string &rank) const {
    for (;; t = taxonNode(t)->parentTaxId) {
      if (ranks.at(taxonNode(t)->rankIdx) == rank) return t;
      if (taxonNode(t)->parentTaxId == t) return t;
    }
  }
};
"""

# stdin: R and R rank strings on their own lines (a rank may be empty or hold a blank), then
# "fmt nNodes euk", the nodes "taxid parent rankIdx", "nParams" and the sets "seqMode accessionLevel minConsCnt
# minConsCntEuk tieRatioBits syncmer smerLen minScoreBits minSpScoreBits em", "nReads" and per read "ql1 ql2 n"
# with n matches "frame pos target species dna reh ham", "nDna" and per case "fmt frame query n targets...".
# stdout: the matches in compareMatches order "seq frame pos target species dna reh ham"; per set and read
# "isClassified classification scoreBits hammingDist nTaxCnt (tax cnt)* top nS2 (species scoreBits)*"
# (top = -1 without a species2Score list); per compareDna case "k (index sum hammings)*".
DRIVER = r"""
static unsigned fb(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static float bf(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
int main() {
  std::string line;
  std::getline(std::cin, line);
  const int R = std::stoi(line);
  TaxonomyWrapper tax;
  for (int i = 0; i < R; i++) { std::getline(std::cin, line); tax.ranks.push_back(line); }
  int fmt, nNodes, euk;
  std::cin >> fmt >> nNodes >> euk;
  tax.euk = euk;
  for (int i = 0; i < nNodes; i++) {
    TaxonNode n; std::cin >> n.taxId >> n.parentTaxId >> n.rankIdx;
    if ((size_t)n.taxId >= tax.row.size()) tax.row.resize(n.taxId + 1, -1);
    tax.row[n.taxId] = (int)tax.nodes.size();
    tax.nodes.push_back(n);
  }
  int nPar; std::cin >> nPar;
  std::vector<LocalParameters> pars(nPar);
  for (auto &p : pars) {
    unsigned tie, ms, mss; int em;
    std::cin >> p.seqMode >> p.accessionLevel >> p.minConsCnt >> p.minConsCntEuk >> tie >> p.syncmer >> p.smerLen >> ms >> mss >> em;
    p.tieRatio = bf(tie); p.minScore = bf(ms); p.minSpScore = bf(mss); p.em = em != 0;
  }
  size_t nReads; std::cin >> nReads;
  std::vector<int> ql1(nReads), ql2(nReads);
  std::vector<Match> ms;
  for (size_t r = 0; r < nReads; r++) {
    size_t n; std::cin >> ql1[r] >> ql2[r] >> n;
    for (size_t k = 0; k < n; k++) {
      Match m; unsigned frame, pos, dna, reh, ham;
      std::cin >> frame >> pos >> m.targetId >> m.speciesId >> dna >> reh >> ham;
      m.qInfo.sequenceID = (uint32_t)r + 1; m.qInfo.frame = (uint8_t)frame; m.qInfo.pos = pos;
      m.dnaEncoding = dna; m.rightEndHamming = (uint16_t)reh; m.hamming = (uint8_t)ham;
      ms.push_back(m);
    }
  }
  std::sort(ms.begin(), ms.end(), KmerMatcher::compareMatches);
  for (auto &m : ms)
    printf("%u %u %u %d %d %u %u %u\n", m.qInfo.sequenceID, (unsigned)m.qInfo.frame, m.qInfo.pos, m.targetId, m.speciesId,
           m.dnaEncoding, (unsigned)m.rightEndHamming, (unsigned)m.hamming);
  for (auto &par : pars) {
    Taxonomer t(par, &tax, fmt);
    std::vector<Query> q(nReads + 1);
    for (size_t r = 0; r < nReads; r++) { q[r + 1].queryLength = ql1[r]; q[r + 1].queryLength2 = ql2[r]; }
    size_t i = 0;
    while (i < ms.size()) {  // one block per read, as Taxonomer::assignTaxonomy cuts them
      const uint32_t cur = ms[i].qInfo.sequenceID;
      const size_t start = i;
      while (i < ms.size() && ms[i].qInfo.sequenceID == cur) ++i;
      t.chooseBestTaxon(cur, start, i - 1, ms.data(), q, par);
    }
    for (size_t r = 1; r <= nReads; r++) {
      const Query &x = q[r];
      printf("%d %d %u %d %zu", (int)x.isClassified, x.classification, fb(x.score), x.hammingDist, x.taxCnt.size());
      for (auto &kv : x.taxCnt) printf(" %d %d", kv.first, kv.second);
      printf(" %d %zu", x.species2Score.empty() ? -1 : x.topSpeciesId, x.species2Score.size());
      for (auto &kv : x.species2Score) printf(" %d %u", kv.first, fb(kv.second));
      printf("\n");
    }
  }
  size_t nDna; std::cin >> nDna;
  for (size_t c = 0; c < nDna; c++) {
    KmerMatcher km; unsigned frame; unsigned long long query; size_t n;
    std::cin >> km.kmerFormat >> frame >> query >> n;
    std::vector<uint64_t> targets(n);
    for (auto &v : targets) { unsigned long long x; std::cin >> x; v = x; }
    std::vector<uint8_t> hd, selSum(n); std::vector<size_t> sel(n); std::vector<uint16_t> selHam(n);
    size_t k = 0;
    km.compareDna(query, targets, hd, sel, selSum, selHam, k, (uint8_t)frame);
    printf("%zu", k);
    for (size_t j = 0; j < k; j++) printf(" %zu %u %u", sel[j], (unsigned)selSum[j], (unsigned)selHam[j]);
    printf("\n");
  }
  return 0;
}
"""


# ---------------------------------------------------------------------------------------------------
# the cases
class Tax:
    def __init__(self, taxo):
        self.taxid = taxo.taxid.tolist()
        self.parent = dict(zip(self.taxid, taxo.parent.tolist()))
        self.rank = dict(zip(self.taxid, taxo.rank))
        self.euk = next(t for t, n in zip(self.taxid, taxo.name) if n == "Eukaryota")
        self.kids = {}
        for t in self.taxid:
            if self.parent[t] != t:
                self.kids.setdefault(self.parent[t], []).append(t)
        self.species = [t for t in self.taxid if self.rank[t] == "species"]

    def strains(self, sp):
        return self.kids.get(sp, [])

    def leaves(self, sp):
        """The deepest nodes under a species (accession leaves on an accession-level DB)."""
        out = []
        for s in self.strains(sp):
            out += self.kids.get(s, [s])
        return out


def reh_of(rng, p_mis):
    """A rightEndHamming word (eight 2-bit codon distances) and its sum, at most 7."""
    f = np.where(rng.random(8) < p_mis, rng.integers(1, 4, 8), 0)
    while f.sum() > 7:
        f[np.argmax(f)] = 0
    return int(sum(int(x) << (2 * i) for i, x in enumerate(f))), int(f.sum())


def chain(rng, fmt, sp, targets, frame, pos0, shifts, ncand=None, p_mis=0.1, extra=None, twins=False):
    """Matches of one (species, frame) group whose DNA encodings are consecutive along `shifts`
    (codons per step) in the direction getMatchPaths checks for this format and frame. ncand[j]
    candidates at position j: the further ones differ from the first in codons that keep them
    consecutive towards one side only, in the middle (towards neither), or not at all. extra[j]: bases
    added to step j (a step that is no multiple of 3). twins: every position holds the same k-mer
    twice with equal hammings, once per target."""
    n, T = len(shifts) + 1, int(sum(shifts))
    c = rng.integers(0, 8, T + 8)

    def enc(u, cod):
        return sum(int(cod[u + i]) << (3 * (7 - i) if fmt == 2 else 3 * i) for i in range(8))

    rows, pos, t = [], pos0, 0
    for j in range(n):
        u = t if frame < 3 else T - t
        reh, ham = reh_of(rng, p_mis)
        if twins:
            for tg in targets:
                rows.append((frame, pos, tg, sp, enc(u, c), reh, ham))
        else:
            for v in range(1 if ncand is None else int(ncand[j])):
                cod = c.copy()
                if v > 0:
                    s = max(1, int(shifts[min(j, n - 2)])) if n > 1 else 1
                    mode = int(rng.integers(0, 4))
                    idx = (u + int(rng.integers(0, s)) if mode == 0 else u + 7 - int(rng.integers(0, s)) if mode == 1
                           else u + 3 + int(rng.integers(0, 2)) if mode == 2 else -1)
                    if idx >= 0:
                        cod[idx] = (cod[idx] + int(rng.integers(1, 8))) % 8
                    if rng.random() < 0.5:
                        reh, ham = reh_of(rng, p_mis)
                rows.append((frame, pos, targets[int(rng.integers(len(targets)))], sp, enc(u, cod), reh, ham))
        if j < n - 1:
            pos += 3 * int(shifts[j]) + (int(extra[j]) if extra is not None else 0)
            t += int(shifts[j])
    return rows


def tie_fork(rng, fmt, sp, targets, frame, pos0):
    """Five matches at four positions: two candidates at the second position, both consecutive to the
    third, with equal path scores (24) but different histories: one extends the first position's match
    (score 21, two codons at distance 1), the other starts there. Through the first the last path
    reaches depth 4, through the second depth 3: the strict `>` on bestScore (the first of the tied
    wins, in compareMatches order) decides whether the group yields a path."""
    c = rng.integers(0, 8, 11)
    alt = c.copy()

    def enc(u, cod):
        return sum(int(cod[u + i]) << (3 * (7 - i) if fmt == 2 else 3 * i) for i in range(8))

    rows = []
    for j in range(4):
        u = j if frame < 3 else 3 - j
        rows.append((frame, pos0 + 3 * j, targets[0], sp, enc(u, c), 0b0101 if j == 0 else 0, 2 if j == 0 else 0))
        if j == 1:  # the codon the step to the third position does not compare
            free = u if frame < 3 else u + 7
            alt[free] = (alt[free] + int(rng.integers(1, 8))) % 8
            rows.append((frame, pos0 + 3, targets[-1], sp, enc(u, alt), 0, 0))
    return rows


def read(tag, ql1, ql2, *row_lists):
    rows = [r for rl in row_lists for r in rl]
    return {"tag": tag, "ql1": ql1, "ql2": ql2, "rows": rows}


def depth_shifts(depth, max_shift, rng=None):
    """Shifts of a chain whose last path has exactly `depth` (depth = 1 + sum of the shifts)."""
    left, out = depth - 1, []
    while left > 0:
        s = min(left, max_shift if rng is None else int(rng.integers(1, max_shift + 1)))
        out.append(s)
        left -= s
    return out


def synthetic_cases(rng, tx, fmt, syn, acc):
    S = tx.species
    ms = 3 if syn else 1  # maxCodonShift at s = 5
    ones = lambda k: depth_shifts(k, ms)  # noqa: E731
    out = []
    lf = lambda sp: tx.leaves(sp)  # noqa: E731
    # forward and reverse frames, 1-3 candidates per position
    for f in range(6):
        for rep in range(2):
            sh = depth_shifts(10, ms, rng)
            out.append(read(f"frame{f}", 150, 150, chain(rng, fmt, S[f], lf(S[f]), f, f % 3, sh,
                                                          ncand=rng.integers(1, 4, len(sh) + 1))))
    # groups of 1 and 2 matches; groups at one position
    good = lambda sp, f=0, p=0: chain(rng, fmt, sp, lf(sp), f, p, ones(12), p_mis=0.05)  # noqa: E731
    out.append(read("group1_only", 150, 150, chain(rng, fmt, S[0], lf(S[0]), 0, 0, []),
                    chain(rng, fmt, S[0], lf(S[0]), 4, 31, []), chain(rng, fmt, S[1], lf(S[1]), 2, 62, [])))
    out.append(read("group12", 150, 150, chain(rng, fmt, S[0], lf(S[0]), 0, 0, []),
                    chain(rng, fmt, S[0], lf(S[0]), 1, 4, [1]), good(S[1], 3, 60)))
    out.append(read("group2_only", 150, 0, chain(rng, fmt, S[2], lf(S[2]), 5, 5, [1])))
    out.append(read("onepos_only", 150, 150, chain(rng, fmt, S[0], lf(S[0]), 0, 30, [], ncand=[4])))
    out.append(read("onepos", 150, 150, chain(rng, fmt, S[0], lf(S[0]), 0, 30, [], ncand=[5]),
                    chain(rng, fmt, S[0], lf(S[0]), 3, 90, [], ncand=[2]), good(S[1], 1, 1)))
    # 2-6 candidates on both sides of every step: tied predecessors
    for k in range(2, 7):
        for rep in range(4):
            f = int(rng.integers(0, 6))
            sh = depth_shifts(int(rng.integers(5, 14)), ms, rng)
            out.append(read(f"cand{k}", 150, 150, chain(rng, fmt, S[rep], lf(S[rep]), f, f % 3, sh,
                                                         ncand=[k] * (len(sh) + 1), p_mis=0.08)))
    for f in range(6):
        for rep in range(3):
            out.append(read("tie_fork", 150, 150, tie_fork(rng, fmt, S[rep], lf(S[rep]), f, 30 + f % 3)))
    # steps that are no multiple of 3, and steps of 1 and 2 bases (shift 0)
    for f in (0, 4):
        sh = ones(9)
        ex = np.zeros(len(sh), int)
        ex[len(sh) // 2] = 1 + f % 2
        out.append(read("step_not3", 150, 150, chain(rng, fmt, S[3], lf(S[3]), f, 3, sh, extra=ex,
                                                     ncand=rng.integers(1, 3, len(sh) + 1))))
        sh0 = ones(5) + [0] + ones(5)
        ex0 = np.zeros(len(sh0), int)
        ex0[len(ones(5))] = 2
        out.append(read("step_lt3", 150, 150, chain(rng, fmt, S[3], lf(S[3]), f, 3, sh0, extra=ex0)))
    # every shift up to maxCodonShift + 1 (syncmer: 1, 2, 3, 4; otherwise 1 and 2)
    for s in range(1, ms + 2):
        for f in (1, 5):
            out.append(read(f"shift{s}", 150, 150, chain(rng, fmt, S[4], lf(S[4]), f, 1, [s] * 6, p_mis=0.05,
                                                         ncand=rng.integers(1, 3, 7))))
            out.append(read(f"shift{s}_mixed", 150, 150,
                            chain(rng, fmt, S[4], lf(S[4]), f, 1, ones(6) + [s] + ones(6), p_mis=0.05)))
    # MIN_DEPTH: the Eukaryota node itself as species (depths 4-8 and 9), Bacteria with 3 and 4
    for d in range(4, 10):
        for f in (0, 3):
            out.append(read(f"euk_depth{d}", 78, 0, chain(rng, fmt, tx.euk, [tx.euk], f, 0, ones(d), p_mis=0.0)))
    for d in (3, 4):
        for f in (2, 4):
            out.append(read(f"bact_depth{d}", 150, 150, chain(rng, fmt, S[5], lf(S[5]), f, 2, ones(d), p_mis=0.0)))
    # a species score above 1.0 before the clamp: a perfect chain over both mates and the gap
    step = ms
    out.append(read("clamp", 150, 150, chain(rng, fmt, S[6], lf(S[6]), 0, 0, [step] * (279 // (3 * step)), p_mis=0.0)))
    # minScore 0.15 at read length 600: 3 * (7 + depth) / 600
    d_of = lambda codons: ones(codons - 7)  # noqa: E731
    perfect = lambda sp, f, p, codons: chain(rng, fmt, sp, lf(sp), f, p, d_of(codons), p_mis=0.0)  # noqa: E731
    out.append(read("minscore_below_above", 300, 300, perfect(S[0], 0, 0, 20), perfect(S[1], 1, 1, 80)))
    out.append(read("minscore_edge", 300, 300, perfect(S[0], 0, 0, 29), perfect(S[1], 1, 1, 30)))
    out.append(read("minscore_edge2", 300, 300, perfect(S[2], 3, 0, 30), perfect(S[1], 1, 1, 29)))
    out.append(read("minscore_only_below", 300, 300, perfect(S[0], 0, 0, 25)))
    # tieRatio 0.95 at read length 600: best 60 codons; 57-59 within, 56 just outside
    out.append(read("tie2", 300, 300, perfect(S[0], 0, 0, 60), perfect(S[1], 1, 1, 58)))
    out.append(read("tie3", 300, 300, perfect(S[0], 0, 0, 59), perfect(S[1], 1, 1, 60), perfect(S[7], 5, 2, 58)))
    out.append(read("tie_outside", 300, 300, perfect(S[0], 0, 0, 60), perfect(S[1], 1, 1, 56)))
    out.append(read("tie_edge", 300, 300, perfect(S[0], 0, 0, 60), perfect(S[1], 1, 1, 57)))
    out.append(read("tie2_outside", 300, 300, perfect(S[2], 0, 0, 56), perfect(S[8], 4, 1, 60),
                    perfect(S[9], 2, 2, 59)))
    # filterRedundantMatches: two strains at one quotient with equal hamming; a lower hamming second
    for sp in (S[0], S[5]):
        out.append(read("twins", 150, 150, chain(rng, fmt, sp, lf(sp)[:2], 0, 0, ones(10), twins=True, p_mis=0.1)))
        out.append(read("lower_second", 150, 150,
                        chain(rng, fmt, sp, lf(sp)[:1], 0, 0, ones(10), p_mis=0.5),
                        chain(rng, fmt, sp, lf(sp)[1:2], 1, 1, ones(10), p_mis=0.0)))
    # BFS: unique best child down to the leaf, two tied children, best child at the threshold
    # (queryLength - 1) / denominator for both denominators (300 / 100 and 2500 / 1000: 2)
    sp = S[3]
    a, b = lf(sp)[0], lf(sp)[-1]
    out.append(read("bfs_unique", 150, 150, chain(rng, fmt, sp, [a], 0, 0, ones(12))))
    for ql1, ql2 in ((150, 150), (2500, 0)):
        for tg in ([a, a, b, sp], [a, a, a, b], [a, b, b, a], [a, a, b, b]):  # four positions, four quotients
            rows = chain(rng, fmt, sp, [a], 0, 0, [ms] * 3, p_mis=0.0)
            rows = [(r[0], r[1], tg[i % 4], *r[3:]) for i, r in enumerate(rows)]
            out.append(read(f"bfs_threshold_{ql1}", ql1, ql2, rows))
    rows = chain(rng, fmt, sp, [a], 3, 0, [ms] * 7)  # eight positions, eight quotients
    out.append(read("bfs_tied", 150, 150, [(r[0], r[1], (a, b)[i % 2], *r[3:]) for i, r in enumerate(rows)]))
    if acc:  # strain-level and species-level targets next to accession leaves
        st = tx.strains(sp)
        rows = chain(rng, fmt, sp, [a], 1, 1, ones(12))
        out.append(read("acc_mixed", 150, 150, [(r[0], r[1], (a, st[0], sp, st[-1])[i % 4], *r[3:])
                                                for i, r in enumerate(rows)]))
    return out


def large_cases(rng, tx, fmt):
    """Sizes at which the kernels change form; fmt2 only."""
    S = tx.species
    lf = tx.leaves
    out = []
    for n in (255, 256, 257, 1023, 1025):  # one (species, frame) group
        out.append(read(f"group{n}", 3 * n + 30, 0, chain(rng, fmt, S[1], lf(S[1]), n % 6, 0, [1] * (n - 1))))
    for n in (512, 513, 2048, 2049):  # matches per read, over six frames and two species
        parts = [n // 6 + (i < n % 6) for i in range(6)]
        rows = []
        for f, k in enumerate(parts):
            rows += chain(rng, fmt, S[2 + f % 2], lf(S[2 + f % 2]), f, f % 3, [1] * (k - 1))
        out.append(read(f"read{n}", 3 * max(parts) + 30, 0, rows))
    rows = chain(rng, fmt, S[4], lf(S[4]), 0, 0, [1] * 4199) + chain(rng, fmt, S[4], lf(S[4]), 4, 1, [1] * 3992)
    out.append(read("read8193", 12700, 0, rows))  # more than 4096 quotients too
    out.append(read("pair_quot160", 250, 250, chain(rng, fmt, S[5], lf(S[5]), 1, 0, [1] * 159)))
    for k in (23, 24, 25):  # paths of one species
        rows = []
        for i in range(k):
            rows += chain(rng, fmt, S[6], lf(S[6]), i % 6, 60 * i + i % 3, [1, 1, 1], p_mis=0.05)
        out.append(read(f"paths{k}", 60 * k + 60, 0, rows))
    return out


def wide_cases(rng, tx, fmt):
    """The `wide` DB (tests/ref_assign_fixture.py): species that really sit under Eukaryota, and reads
    whose taxCnt holds 64 / 65 and 256 / 257 distinct taxa (one strain per position and quotient)."""
    S = tx.species
    out = []
    wide_sp = max(S, key=lambda sp: len(tx.strains(sp)))
    kids = tx.strains(wide_sp)
    for n in (64, 65, 256, 257):
        for f in (0, 4):
            rows = chain(rng, fmt, wide_sp, kids[:1], f, 0, [1] * (n - 1), p_mis=0.02)
            rows = [(r[0], r[1], kids[i], *r[3:]) for i, r in enumerate(rows)]
            out.append(read(f"taxa{n}", *((150, 150) if n < 100 else (900, 0)), rows))
    under = [sp for sp in S if is_under(tx, sp, tx.euk)]
    assert under and tx.euk not in under
    for d in range(4, 10):
        for f in (0, 3):
            sp = under[(d + f) % len(under)]
            out.append(read(f"eukspecies_depth{d}", 78, 0, chain(rng, fmt, sp, tx.leaves(sp), f, 0, [1] * (d - 1), p_mis=0.0)))
            out.append(read(f"euk_depth{d}", 78, 0, chain(rng, fmt, tx.euk, [tx.euk], f, 0, [1] * (d - 1), p_mis=0.0)))
    for f in range(6):  # a Eukaryota species next to a bacterial one, both with paths
        sp = under[f % len(under)]
        out.append(read("euk_and_bacteria", 150, 150, chain(rng, fmt, sp, tx.leaves(sp), f, f % 3, [1] * 11, p_mis=0.05),
                        chain(rng, fmt, S[1], tx.leaves(S[1]), (f + 1) % 6, 60, [1] * 6, p_mis=0.05)))
    return out


def is_under(tx, t, anc):
    while t != anc and tx.parent[t] != t:
        t = tx.parent[t]
    return t == anc


def real_cases(db_dir, gen, base_par):
    """The oracle's extract + match on synthetic reads, split by read."""
    from metabuli_work_amd import synth
    from metabuli_work_amd._abi import info_frame, info_pos, info_seq
    from tests import oracle_ctypes as oc
    out = []
    odb = oc.OracleDb(db_dir)
    for kind in ("paired", "long"):
        par = base_par(2 if kind == "paired" else 3)
        if kind == "paired":
            reads = synth.make_reads(gen, 60, paired=True, seed=5, short_frac=0.03, rate_n=0.002, rate_iupac=0.001,
                                     rate_lower=0.002)
        else:
            reads = synth.make_long_reads(gen, 3, n50=1500, min_len=400, seed=5)
        kmers, ql1, ql2 = oc.extract(par, reads)
        m = oc.match(odb, par, kmers)
        seq = info_seq(m["qinfo"]).astype(np.int64)
        for r in range(reads.n):
            x = m[seq == r + 1]
            rows = list(zip(info_frame(x["qinfo"]).tolist(), info_pos(x["qinfo"]).tolist(), x["target_id"].tolist(),
                            x["species_id"].tolist(), x["dna_encoding"].tolist(), x["right_end_hamming"].tolist(),
                            x["hamming"].tolist()))
            out.append(read(f"real_{kind}", int(ql1[r]), int(ql2[r]), rows))
    odb.close()
    return out


def dna_cases(rng):
    """compareDna: lists of 1-40 candidates equal in AA, with 0-8 changed codons each."""
    out = []
    for fmt in (1, 2):
        for frame in range(6):
            for rep in range(60):
                n = int(rng.integers(1, 41)) if rep % 6 else (1, 2, 40)[rep // 6 % 3]
                q = int(rng.integers(0, 1 << 62))
                floor = int(rng.integers(0, 6))  # changed codons of the closest candidate
                tg = []
                one = rep % 10 == 3  # the whole list at one distance: one k-mer repeated
                base = None
                for _ in range(n):
                    if one and base is not None:
                        tg.append(base)
                        continue
                    k = floor + (int(rng.integers(0, 4)) if rng.random() < 0.7 else 0)
                    t = q
                    for i in rng.permutation(8)[:min(k, 8)]:
                        cod = (t >> (3 * int(i))) & 7
                        t = (t & ~(7 << (3 * int(i)))) | (((cod + int(rng.integers(1, 8))) % 8) << (3 * int(i)))
                    base = t
                    tg.append(t)
                out.append((fmt, frame, q, tg))
    return out


# ---------------------------------------------------------------------------------------------------
def build_all():
    from metabuli_work_amd import synth
    from metabuli_work_amd._abi import default_params
    from tests import oracle_ctypes as oc
    from tests.conftest import DB_CONFIGS
    from tests.ref_assign_fixture import WIDE, WIDE_CONFIG, build_wide_db

    ranks = []
    jobs = {}
    tmp = tempfile.TemporaryDirectory()
    for name in DBS + [WIDE]:
        d = str(pathlib.Path(tmp.name) / name)
        if name == WIDE:
            fmt, syn, acc = WIDE_CONFIG["kmer_format"], 0, 0
            taxo = build_wide_db(d)
        else:
            fmt, syn, nsp, nst, glen, *ex = DB_CONFIGS[name]
            ex = ex[0] if ex else {}
            acc = ex.get("accessions", 0)
            taxo = synth.make_taxonomy(nsp, nst, seed=11, accessions=acc)
            gen = synth.make_genomes(taxo, genome_len=glen, seed=12, species_div=ex.get("species_div", 0.0))
            oc.build_db(d, default_params(kmer_format=fmt, syncmer=syn, smer_len=5, accession_level=1 if acc else 0),
                        taxo, gen)

        def base_par(seq_mode, acc_level=0, d=d):
            return oc.load_db_parameters(d, default_params(seq_mode=seq_mode, accession_level=acc_level))

        pars = []
        for seq_mode, acc_level, min_score, min_sp, em in PARAM_SETS:
            p = base_par(seq_mode, acc_level)
            pars.append([p.seq_mode, p.accession_level, p.min_cons_cnt, p.min_cons_cnt_euk, fbits(p.tie_ratio), p.syncmer,
                         p.smer_len, fbits(min_score), fbits(min_sp), em, p.kmer_format])
        rng = np.random.default_rng([20261022, (DBS + [WIDE]).index(name)])
        tx = Tax(taxo)
        if name == WIDE:
            cases = wide_cases(rng, tx, fmt)
        else:
            cases = real_cases(d, gen, base_par) + synthetic_cases(rng, tx, fmt, syn, acc)
        if name == "fmt2":
            cases += large_cases(rng, tx, fmt)
        empty = read("empty", 150, 150, [])
        mid = len(cases) // 2
        cases = [empty] + cases[:mid] + [empty, empty, empty] + cases[mid:] + [empty]
        for r in taxo.rank:
            if r not in ranks:
                ranks.append(r)
        jobs[name] = dict(fmt=fmt, syn=syn, taxo=taxo, tx=tx, pars=pars, cases=cases)
    if "" not in ranks:
        ranks.append("")
    # fmt2_acc_blank: the fmt2_acc taxonomy with the strains' rank strings emptied, its own small case set
    j = jobs["fmt2_acc"]
    rng = np.random.default_rng([20261022, 99])
    blank = dict(j)
    blank["blank"] = True
    blank["cases"] = [c for c in synthetic_cases(rng, j["tx"], j["fmt"], j["syn"], True)
                      if c["tag"].startswith(("bfs", "acc", "twins", "lower", "frame"))]
    jobs["fmt2_acc_blank"] = blank
    tmp.cleanup()
    return ranks, jobs


def check_bounds(job):
    """Every pos / dnaShift inside filterRedundantMatches' arrays; IDs inside the tree; targets under species."""
    tx = job["tx"]
    dna_shift = 9 if job["syn"] else 3
    for c in job["cases"]:
        ql = c["ql1"] + c["ql2"]
        for f, pos, tg, sp, dna, reh, ham in c["rows"]:
            assert 0 <= f < 6 and 0 <= pos and pos // dna_shift <= (ql + 3) // dna_shift, (c["tag"], pos, ql)
            assert tg in tx.parent and sp in tx.parent and tg != 0 and sp != 0
            t = tg
            while t != sp:
                assert tx.parent[t] != t, (c["tag"], tg, sp)
                t = tx.parent[t]
            assert 0 <= dna < (1 << 24) and 0 <= reh < (1 << 16) and 0 <= ham < 256


def job_input(ranks, job, dna):
    taxo = job["taxo"]
    lines = [str(len(ranks))] + ranks
    lines.append(f"{job['fmt']} {len(taxo.taxid)} {job['tx'].euk}")
    for t, p, r in zip(taxo.taxid.tolist(), taxo.parent.tolist(), taxo.rank):
        if job.get("blank") and r == "no rank" and t != 1:
            r = ""
        lines.append(f"{t} {p} {ranks.index(r)}")
    lines.append(str(len(job["pars"])))
    lines += [" ".join(str(x) for x in p[:10]) for p in job["pars"]]
    lines.append(str(len(job["cases"])))
    for c in job["cases"]:
        lines.append(f"{c['ql1']} {c['ql2']} {len(c['rows'])}")
        lines += [" ".join(str(int(x)) for x in r) for r in c["rows"]]
    lines.append(str(len(dna)))
    for fmt, frame, q, tg in dna:
        lines.append(f"{fmt} {frame} {q} {len(tg)} " + " ".join(str(t) for t in tg))
    return "\n".join(lines) + "\n"


def parse(job, dna, text, name, ranks, arrays):
    it = iter(text.split("\n"))
    n_m = sum(len(c["rows"]) for c in job["cases"])
    m = np.array([[int(x) for x in next(it).split()] for _ in range(n_m)], np.int64).reshape(-1, 8)
    taxo = job["taxo"]
    rank = ["" if job.get("blank") and r == "no rank" and t != 1 else r for t, r in zip(taxo.taxid.tolist(), taxo.rank)]
    a = arrays
    a[f"{name}_tax_id"] = taxo.taxid.astype(np.int32)
    a[f"{name}_tax_parent"] = taxo.parent.astype(np.int32)
    a[f"{name}_tax_rank"] = np.array([ranks.index(r) for r in rank], np.uint8)
    a[f"{name}_euk"] = np.int32(job["tx"].euk)
    a[f"{name}_params"] = np.array(job["pars"], np.int64)
    a[f"{name}_m_qinfo"] = (m[:, 2].astype(np.uint64) | (m[:, 0].astype(np.uint64) << np.uint64(32)) |
                            (m[:, 1].astype(np.uint64) << np.uint64(61)))
    a[f"{name}_m_target"] = m[:, 3].astype(np.uint32)
    a[f"{name}_m_species"] = m[:, 4].astype(np.uint32)
    a[f"{name}_m_dna"] = m[:, 5].astype(np.uint32)
    a[f"{name}_m_reh"] = m[:, 6].astype(np.uint16)
    a[f"{name}_m_ham"] = m[:, 7].astype(np.uint8)
    a[f"{name}_ql1"] = np.array([c["ql1"] for c in job["cases"]], np.uint32)
    a[f"{name}_ql2"] = np.array([c["ql2"] for c in job["cases"]], np.uint32)
    a[f"{name}_tag"] = np.array([c["tag"] for c in job["cases"]])
    for p in range(len(job["pars"])):
        res, tcl, tc, top, s2l, s2 = [], [], [], [], [], []
        for _ in job["cases"]:
            v = [int(x) for x in next(it).split()]
            res.append(v[:4])
            k = v[4]
            tcl.append(k)
            tc += [v[5 + 2 * i:7 + 2 * i] for i in range(k)]
            o = 5 + 2 * k
            top.append(v[o])
            s2l.append(v[o + 1])
            s2 += [v[o + 2 + 2 * i:o + 4 + 2 * i] for i in range(v[o + 1])]
            assert len(v) == o + 2 + 2 * v[o + 1]
        res = np.array(res, np.int64)
        a[f"{name}_p{p}_is_classified"] = res[:, 0].astype(np.uint8)
        a[f"{name}_p{p}_classification"] = res[:, 1].astype(np.int32)
        a[f"{name}_p{p}_score_bits"] = res[:, 2].astype(np.uint32)
        a[f"{name}_p{p}_hamming_dist"] = res[:, 3].astype(np.int32)
        a[f"{name}_p{p}_tc_len"] = np.array(tcl, np.uint32)
        a[f"{name}_p{p}_tc"] = np.array(tc, np.int64).reshape(-1, 2).astype(np.int32)
        if job["pars"][p][9]:
            a[f"{name}_p{p}_top"] = np.array(top, np.int32)
            a[f"{name}_p{p}_s2_len"] = np.array(s2l, np.uint32)
            a[f"{name}_p{p}_s2"] = np.array(s2, np.int64).reshape(-1, 2)
    if dna:
        k, sel = [], []
        for _ in dna:
            v = [int(x) for x in next(it).split()]
            k.append(v[0])
            sel += [v[1 + 3 * i:4 + 3 * i] for i in range(v[0])]
        a["dna_fmt"] = np.array([d[0] for d in dna], np.uint8)
        a["dna_frame"] = np.array([d[1] for d in dna], np.uint8)
        a["dna_query"] = np.array([d[2] for d in dna], np.uint64)
        a["dna_n"] = np.array([len(d[3]) for d in dna], np.uint32)
        a["dna_targets"] = np.array([t for d in dna for t in d[3]], np.uint64)
        a["dna_k"] = np.array(k, np.uint32)
        a["dna_sel"] = np.array(sel, np.int64).reshape(-1, 3).astype(np.uint32)


def generate():
    ranks, jobs = build_all()
    dna = dna_cases(np.random.default_rng(20261023))
    arrays = {"rank_names": np.array(ranks), "param_cols": np.array(PARAM_COLS), "dbs": np.array(list(jobs))}
    with tempfile.TemporaryDirectory() as d:
        src = pathlib.Path(d) / "ref_assign.cpp"
        src.write_text(program())
        flags = ["-O1", "-std=c++17", "-ffp-contract=off", "-w", f"-I{REF}", str(src)]
        exe, san = pathlib.Path(d) / "ref_assign", pathlib.Path(d) / "ref_assign_san"
        subprocess.run(["g++", *flags, "-o", str(exe)], check=True)
        subprocess.run(["g++", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *flags, "-o", str(san)],
                       check=True)
        for name, job in jobs.items():
            check_bounds(job)
            inp = job_input(ranks, job, dna if name == "fmt2" else [])
            got = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, check=True).stdout
            chk = subprocess.run([str(san)], input=inp, capture_output=True, text=True)
            assert chk.returncode == 0 and chk.stderr == "", (name, chk.returncode, chk.stderr[-2000:])
            assert chk.stdout == got, f"{name}: the sanitised build printed something else"
            parse(job, dna if name == "fmt2" else [], got, name, ranks, arrays)
            print(name, len(job["cases"]), "reads,", len(arrays[f"{name}_m_ham"]), "matches: sanitised run clean")
    return arrays


if __name__ == "__main__":
    arrays = generate()
    out = HERE / "ref_assign.npz"
    np.savez_compressed(out, **arrays)
    print("wrote", out, out.stat().st_size, "bytes,", sum(len(arrays[f"{n}_m_ham"]) for n in arrays["dbs"]), "matches")
    sys.path.insert(0, str(ROOT))
    from tests.ref_assign_fixture import coverage_table  # the table test_golden_covers_branches asserts on
    for k, v in coverage_table(np.load(out)).items():
        print(f"{k:40s} {v}")
