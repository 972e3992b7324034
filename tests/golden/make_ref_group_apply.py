"""Regenerate tests/golden/ref_group_apply.npz and group_apply_defaults.json: the reference's OWN
GroupApplier run on a small designed case.

Runs only where the reference tree is mounted; the committed outputs are what the tests read. As in
make_ref_groups.py nothing of the reference enters the repository: the code below is cut out of the
reference's files at run time, pasted into a throw-away C++ file in a temporary directory, compiled, run
and deleted. The cut code:
* GroupApplier.cpp: `loadOrgResult`, `loadGroupsFromFile`, `getRepLabel`, `applyRepLabel`,
  `startGroupApplication`, whole, as written; GroupApplier.h: `struct OrgResult`
* Reporter.cpp: the `group` overload of `writeReadClassification`
* TaxonomyWrapper.cpp: `splitByDelimiter`
* common.h: `struct Query`
next to this project's own declaration-only stubs: a `TaxonomyWrapper` over the designed tree below
(nodes.dmp read with internal taxIDs numbered as TaxonomyWrapper.cpp:148-195 numbers them: from 1, by
first appearance, a row's taxID before its parent's) with `getExternal2internalTaxID`, `getOriginalTaxID`,
`getString`, `taxonNode` and `weightedMajorityLCA`, which is MMseqs2's and absent from the reference
tree: it is RESTATED here from the published algorithm (parity unpinned); a `Reporter` holding the
stream; a `LocalParameters` with the fields the cut code reads.

Every score is a multiple of 1/64, so every sum is exact in float and double and the reference's
unordered_set order cannot change a result; each score is asserted to survive its round trip through the
TSV's text. groupRep is written in unordered_map order there; its lines are sorted by group here.
The same program is also built with -fsanitize=address,undefined (a stand-alone CPU binary) and must
give the same files. group_apply_defaults.json is parsed from the text of setGroupApplicationDefaults.
"""
import json
import pathlib
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
REF = pathlib.Path("/root/reference/src")

from make_ref_functions import definitions  # noqa: E402
from make_ref_groups import block  # noqa: E402

# The designed tree: (taxID, parent, rank) in nodes.dmp order. 32 comes before 31 and 41 before its parent
# 40, so the internal numbering is not the external order; 50 / 51 have no ranked node in their lineage.
NODES = [(1, 1, "no rank"), (10, 1, "superkingdom"), (20, 10, "phylum"), (30, 20, "genus"), (32, 30, "species"),
         (31, 30, "species"), (33, 31, "no rank"), (41, 40, "species"), (40, 20, "genus"), (7, 40, "species"),
         (50, 1, "no rank"), (51, 50, "no rank"), (60, 1, "superkingdom"), (61, 60, "species")]

# (group, label, score x 64) per read, in read order; group = the smallest read ID of the group, 0 = none
READS = [
    (1, 31, 32), (1, 31, 16), (1, 32, 8),                 # a plain majority
    (4, 31, 32), (4, 32, 32), (4, 0, 0), (4, 31, 9),      # two sibling species at exactly 0.5; a low scorer; label 0
    (8, 41, 48), (8, 7, 16),                              # a child listed before its parent
    (10, 31, 16), (10, 41, 16),                           # species of two genera at 0.5 each; scores at 0.25
    (12, 31, 16), (12, 41, 16), (12, 7, 16),              # an LCA (genus 40) holds 2/3
    (15, 1, 32), (15, 0, 0),                              # every vote on the root
    (17, 51, 16), (17, 31, 16), (17, 61, 16),             # only the root holds half: a representative equal to the root
    (20, 0, 0), (20, 0, 16),                              # no voter at all
    (22, 31, 8), (22, 32, 8),                             # voters only below 0.15
    (0, 31, 32), (0, 0, 0),                               # reads of no group
    (26, 33, 40), (26, 31, 8), (26, 0, 48),               # a label that is an ancestor of another
]

# (weight_mode, min_vote_score): the three modes at the default, thresholds 0, at a score (0.25) and above all
CASES = [(0, 0.15), (1, 0.15), (2, 0.15), (1, 0.0), (2, 0.0), (0, 0.0), (1, 0.25), (2, 0.25), (1, 2.0), (2, 2.0)]

STUBS = r"""
#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>
using namespace std;
typedef int TaxID;
struct Kmer {};
template <typename T> struct Buffer {};
struct LocalParameters {
  int taxidCol, scoreCol, readIdCol, weightMode; float minVoteScr; bool printLineage;
  std::vector<std::string> filenames;
};
struct TaxonNode { int id; TaxID taxId; TaxID parentTaxId; size_t rankIdx; size_t nameIdx; };
struct WeightedTaxHit { TaxID taxon; float weight; WeightedTaxHit(TaxID t, float w, int) : taxon(t), weight(w) {} };
struct WeightedTaxResult { TaxID taxon; };
class TaxonomyWrapper {
 public:
  std::vector<TaxonNode> nodes; std::vector<std::string> strings; std::vector<int> D, internal2org;
  std::unordered_map<int, int> org2internal;
  TaxonomyWrapper(const std::string &namesFile, const std::string &nodesFile, const std::string &mergedFile, bool useInternalTaxID);
  static std::vector<std::string> splitByDelimiter(const std::string &s, const std::string &delimiter, int maxCol);
  void getExternal2internalTaxID(std::unordered_map<int, int> &m) const { m = org2internal; }
  TaxID getOriginalTaxID(TaxID t) const { return internal2org[t]; }
  const char *getString(size_t i) const { return strings[i].c_str(); }
  const TaxonNode *taxonNode(TaxID t) const { return &nodes[D[t]]; }
  std::string taxLineage2(const TaxonNode *) const { return "-"; }
  int findRankIndex(const std::string &r) const;
  WeightedTaxResult weightedMajorityLCA(const std::vector<WeightedTaxHit> &setTaxa, const float majorityCutoff);
};
class Reporter {
 public:
  const LocalParameters &par; TaxonomyWrapper *taxonomy; std::ofstream readClassificationFile; bool isFirstTime = true;
  Reporter(const LocalParameters &par, TaxonomyWrapper *t) : par(par), taxonomy(t) {}
  void openReadClassificationFile(const std::string fileName) { readClassificationFile.open(fileName); }
  void writeReadClassification(const vector<struct Query> &queryList, const vector<uint32_t> &groupIdList, bool classifiedOnly = false);
  void closeReadClassificationFile() { readClassificationFile.close(); }
};
"""

# This project's statements, not the reference's: the stub taxonomy and MMseqs2's weightedMajorityLCA restated.
OWN = r"""
TaxonomyWrapper::TaxonomyWrapper(const std::string &, const std::string &nodesFile, const std::string &, bool) {
  std::ifstream ss(nodesFile); std::string line; int cnt = 0;
  internal2org.push_back(0);
  struct Row { int t, p; std::string r; }; std::vector<Row> rows;
  while (std::getline(ss, line)) {
    std::vector<std::string> f = splitByDelimiter(line, "\t|\t", 3);
    int ids[2] = {atoi(f[0].c_str()), atoi(f[1].c_str())};
    for (int x : ids) if (!org2internal.count(x)) { org2internal[x] = ++cnt; internal2org.push_back(x); }
    rows.push_back({org2internal[ids[0]], org2internal[ids[1]], f[2]});
  }
  D.assign(cnt + 1, -1);
  for (size_t i = 0; i < rows.size(); i++) {
    strings.push_back(rows[i].r);
    nodes.push_back({(int)i, rows[i].t, rows[i].p, strings.size() - 1, 0});
    D[rows[i].t] = (int)i;
  }
}
int TaxonomyWrapper::findRankIndex(const std::string &r) const {
  static const std::map<std::string, int> ranks = {
    {"forma", 1}, {"varietas", 2}, {"subspecies", 3}, {"species", 4}, {"species subgroup", 5}, {"species group", 6},
    {"subgenus", 7}, {"genus", 8}, {"subtribe", 9}, {"tribe", 10}, {"subfamily", 11}, {"family", 12},
    {"superfamily", 13}, {"parvorder", 14}, {"infraorder", 15}, {"suborder", 16}, {"order", 17}, {"superorder", 18},
    {"infraclass", 19}, {"subclass", 20}, {"class", 21}, {"superclass", 22}, {"subphylum", 23}, {"phylum", 24},
    {"superphylum", 25}, {"subkingdom", 26}, {"kingdom", 27}, {"superkingdom", 28}, {"domain", 28}};
  auto it = ranks.find(r);
  return it == ranks.end() ? -1 : it->second;
}
WeightedTaxResult TaxonomyWrapper::weightedMajorityLCA(const std::vector<WeightedTaxHit> &setTaxa, const float majorityCutoff) {
  struct Anc { double weight = 0; bool candidate = false; std::set<TaxID> children; };
  std::map<TaxID, Anc> anc;
  double total = 0;
  for (const WeightedTaxHit &h : setTaxa) {
    total += h.weight;
    const TaxonNode *n = taxonNode(h.taxon);
    TaxID prev = 0; bool first = true;
    for (;;) {
      Anc &a = anc[n->taxId];
      a.weight += h.weight;
      if (first) a.candidate = true;
      else { a.children.insert(prev); if (a.children.size() >= 2) a.candidate = true; }
      if (n->parentTaxId == n->taxId) break;
      prev = n->taxId; first = false; n = taxonNode(n->parentTaxId);
    }
  }
  if (total == 0) return {0};
  const int ROOT_RANK = 2147483647;
  int minRank = ROOT_RANK; TaxID selected = 0; double selectedPercent = 0;
  for (auto &kv : anc) {
    if (!kv.second.candidate) continue;
    const double percent = kv.second.weight / total;
    if (!(percent >= majorityCutoff)) continue;
    int rank = ROOT_RANK;
    for (const TaxonNode *n = taxonNode(kv.first); n->parentTaxId != n->taxId; n = taxonNode(n->parentTaxId)) {
      const int r = findRankIndex(getString(n->rankIdx));
      if (r > 0) { rank = r; break; }
    }
    if (selected == 0 || rank < minRank || (rank == minRank && percent > selectedPercent)) {
      selected = kv.first; minRank = rank; selectedPercent = percent;
    }
  }
  return {selected};
}
class GroupApplier {
 public:
  const LocalParameters &par;
  string groupFileDir, groupmapFileDir, taxDbDir, orgRes, outDir, updatedResultFileName, updatedReportFileName;
  Reporter *reporter = nullptr; TaxonomyWrapper *taxonomy = nullptr;
  GroupApplier(LocalParameters &par) : par(par) {
    groupFileDir = par.filenames[0]; groupmapFileDir = par.filenames[1]; taxDbDir = par.filenames[2];
    orgRes = par.filenames[3]; outDir = par.filenames[4];
    taxonomy = new TaxonomyWrapper(taxDbDir + "/names.dmp", taxDbDir + "/nodes.dmp", taxDbDir + "/merged.dmp", true);
    updatedResultFileName = outDir + "/updated_classifications.tsv";
    reporter = new Reporter(par, taxonomy);
  }
  ~GroupApplier() { delete taxonomy; delete reporter; }
  void startGroupApplication(const LocalParameters &par);
  void loadOrgResult(vector<OrgResult> &orgResults, size_t &processedReadCnt);
  void loadGroupsFromFile(unordered_map<uint32_t, unordered_set<uint32_t>> &groupInfo, vector<uint32_t> &groupMappingInfo,
                          const string &groupInfoFileName, const string &groupMappingInfoFileName);
  void getRepLabel(vector<OrgResult> &orgResults, const unordered_map<uint32_t, unordered_set<uint32_t>> &groupInfo,
                   unordered_map<uint32_t, uint32_t> &repLabel, std::unordered_map<int, int> &external2internalTaxId);
  void applyRepLabel(const vector<OrgResult> &orgResults, const vector<uint32_t> &groupMappingInfo,
                     const unordered_map<uint32_t, uint32_t> &repLabel, std::unordered_map<int, int> &external2internalTaxId);
};
"""

# argv: groups groupMap taxonomy-dir tsv out-dir weightMode minVoteScr-bits
DRIVER = r"""
int main(int argc, char **argv) {
  if (argc != 8) return 9;
  LocalParameters par;
  par.taxidCol = 3; par.scoreCol = 5; par.readIdCol = 2; par.printLineage = false;
  par.weightMode = atoi(argv[6]);
  unsigned bits = (unsigned)strtoul(argv[7], nullptr, 10); memcpy(&par.minVoteScr, &bits, 4);
  for (int i = 1; i <= 5; i++) par.filenames.push_back(argv[i]);
  GroupApplier g(par);
  g.startGroupApplication(par);
  return 0;
}
"""


def program() -> str:
    ga = (REF / "read-group" / "GroupApplier.cpp").read_text()
    gh = (REF / "read-group" / "GroupApplier.h").read_text()
    rp = (REF / "commons" / "Reporter.cpp").read_text()
    tw = (REF / "commons" / "TaxonomyWrapper.cpp").read_text()
    ch = (REF / "commons" / "common.h").read_text()
    methods = []
    for name in ("loadOrgResult", "loadGroupsFromFile", "getRepLabel", "applyRepLabel", "startGroupApplication"):
        d = definitions(ga, rf"void GroupApplier::{name}\(")
        assert len(d) == 1, name
        methods += d
    writer = [d for d in definitions(rp, r"void Reporter::writeReadClassification\(") if "groupIdList" in d]
    split = definitions(tw, r"std::vector<std::string> TaxonomyWrapper::splitByDelimiter\(")
    assert len(writer) == 1 and len(split) == 1
    return "\n".join([STUBS, block(ch, "struct Query {", ";"), block(gh, "struct OrgResult {", ";"), OWN, *split,
                      *writer, *methods, DRIVER])


def inputs():
    """(nodes.dmp, names.dmp, classification TSV, groupMap, groups) of the designed case, bytes / array."""
    nodes = "".join(f"{t}\t|\t{p}\t|\t{r}\t|\t\t|\n" for t, p, r in NODES).encode()
    names = "".join(f"{t}\t|\ttaxon_{t}\t|\t\t|\tscientific name\t|\n" for t, _, _ in NODES).encode()
    rank = {t: r for t, _, r in NODES}
    rows = ["#is_classified\tname\ttaxID\tquery_length\tscore\trank\ttaxID:match_count\n", "\n"]
    for i, (_, lab, s64) in enumerate(READS):
        sc = np.float32(s64 / 64.0)
        text = "%.9g" % float(sc)
        assert np.float32(float(text)) == sc and float(sc) * 64 == s64, (i, text)
        rows.append(f"{1 if lab else 0}\tread_{i + 1}\t{lab}\t150\t{text}\t{rank[lab] if lab else '-'}\t" +
                    (f"{lab}:3 \n" if lab else "-\t\n"))
    gm = np.array([0] + [g for g, _, _ in READS], np.uint32)
    for g in set(gm[1:].tolist()) - {0}:
        assert g == int(np.nonzero(gm == g)[0][0]), "a group's ID is its smallest read ID"
    groups = ""
    for g in sorted(set(gm[1:].tolist()) - {0}):
        groups += f"{g}\t" + "".join(f"{m}\t" for m in np.nonzero(gm == g)[0].tolist()) + "\n"
    return nodes, names, "".join(rows).encode(), gm, groups.encode()


def run_case(exe, d, mode, thr):
    out = pathlib.Path(d) / "out"
    out.mkdir(exist_ok=True)
    for f in out.iterdir():
        f.unlink()
    bits = int(np.float32(thr).view(np.uint32))
    subprocess.run([str(exe), f"{d}/groups", f"{d}/groupMap", f"{d}/taxonomy", f"{d}/classifications.tsv", str(out),
                    str(mode), str(bits)], check=True, stdout=subprocess.DEVNULL)
    rep = sorted((out / "groupRep").read_text().splitlines(), key=lambda ln: int(ln.split("\t")[0]))
    return ("".join(ln + "\n" for ln in rep)).encode(), (out / "updated_classifications.tsv").read_bytes()


def defaults() -> dict:
    text = (REF / "workflow" / "groupApplication.cpp").read_text()
    body = re.sub(r"//[^\n]*", "", block(text, "void setGroupApplicationDefaults("))
    out = {}
    for name, expr in re.findall(r"par\.(\w+)\s*=\s*([^;]+);", body):
        expr = expr.strip()
        out[name] = {"text": expr, "value": float(expr.rstrip("f")) if re.search(r"[.f]", expr) else int(expr)}
    return out


if __name__ == "__main__":
    nodes, names, tsv, gm, groups = inputs()
    arrays = {"nodes_dmp": np.frombuffer(nodes, np.uint8), "names_dmp": np.frombuffer(names, np.uint8),
              "tsv": np.frombuffer(tsv, np.uint8), "group_map": gm, "groups": np.frombuffer(groups, np.uint8),
              "node_taxid": np.array([t for t, _, _ in NODES], np.int32),
              "node_parent": np.array([p for _, p, _ in NODES], np.int32), "node_rank": np.array([r for _, _, r in NODES]),
              "case_mode": np.array([m for m, _ in CASES], np.int32),
              "case_min_vote_score": np.array([t for _, t in CASES], np.float32)}
    with tempfile.TemporaryDirectory() as d:
        p = pathlib.Path(d)
        (p / "taxonomy").mkdir()
        (p / "taxonomy" / "nodes.dmp").write_bytes(nodes)
        (p / "taxonomy" / "names.dmp").write_bytes(names)
        (p / "taxonomy" / "merged.dmp").write_bytes(b"")
        (p / "classifications.tsv").write_bytes(tsv)
        (p / "groups").write_bytes(groups)
        (p / "groupMap").write_text("".join(f"{i}\t{g}\n" for i, g in enumerate(gm[1:].tolist(), 1)))
        src, exe, exe_san = p / "ref_apply.cpp", p / "ref_apply", p / "ref_apply_san"
        src.write_text(program())
        common = ["g++", "-std=c++17", "-Wno-unused-result", "-Wno-sign-compare", str(src)]
        subprocess.run(common + ["-O1", "-o", str(exe)], check=True)
        subprocess.run(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                                 str(exe_san)], check=True)
        for k, (mode, thr) in enumerate(CASES):
            rep, upd = run_case(exe, d, mode, thr)
            assert (rep, upd) == run_case(exe_san, d, mode, thr), f"case {k}: the sanitizer build disagrees"
            arrays[f"case{k}_group_rep"] = np.frombuffer(rep, np.uint8)
            arrays[f"case{k}_updated"] = np.frombuffer(upd, np.uint8)
            print(f"case {k}: mode {mode} min_vote_score {thr}: groupRep", rep.decode().replace("\n", " ").replace("\t", ":"))
    arrays["sanitizer_clean"] = np.array(True)
    np.savez_compressed(HERE / "ref_group_apply.npz", **arrays)
    (HERE / "group_apply_defaults.json").write_text(json.dumps(
        {"source": "src/workflow/groupApplication.cpp: setGroupApplicationDefaults", "defaults": defaults()}, indent=1) + "\n")
    print("wrote", HERE / "ref_group_apply.npz", (HERE / "ref_group_apply.npz").stat().st_size, "bytes")
