"""Regenerate tests/golden/ref_groups.npz and group_defaults.json: the reference's OWN grouping phases
run on the designed edge lists of tests/group_cases.py.

Runs only where the reference tree is mounted; the committed outputs are what the tests read. As in
make_ref_functions.py nothing of the reference enters the repository: the code below is cut out of the
reference's files at run time, pasted into a throw-away C++ file in a temporary directory, compiled
(-fopenmp), run and deleted. The cut code:
* GroupGenerator.h: `struct Relation`, `makeRelation`, `class DisjointSet`, `addSat16`,
  `getRouteRangeSize`, `routeOf`, `M_HIST_BUCKETS`, `mHistBucket`, `capFromQuantile`, `MERGE_SUPPORT_FLOOR`
* GroupGenerator.cpp: `makeGroups`, `mergeBySupport`, `makeGroupsPhase2`, whole, as written
* common.h: `ReadBuffer`, `WriteBuffer`
next to a declaration-only `GroupGenerator` (the three methods, `par`, `outDir`) and a
`LocalParameters` holding `threads`. The driver writes each case's edges as relations_{route}.bin
through the cut WriteBuffer / makeRelation, routed by the cut routeOf (files 0 .. 2 * threads, as the
phases read them), and calls the phases as startGroupGeneration does (GroupGenerator.cpp:199-214),
with 1, 3 and 16 threads; the maps must agree across the thread counts (asserted here, recorded in the
.npz as `threads_agree`). The same program is also built with -fsanitize=address,undefined and run
once over every case (a stand-alone CPU binary); its maps must equal the plain build's.
group_defaults.json is parsed from the text of setGroupGenerationDefaults.
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

from make_ref_functions import _block_end, definitions  # noqa: E402
from tests import group_cases  # noqa: E402


def block(text: str, head: str, tail: str = "") -> str:
    i = text.index(head)
    e = _block_end(text, text.index("{", i))
    if tail:
        assert text[e:e + len(tail)] == tail, text[e:e + 10]
        e += len(tail)
    return text[i:e]


def line_of(text: str, head: str) -> str:
    i = text.index(head)
    return text[i:text.index(";", i) + 1]


def program() -> str:
    gh = (REF / "read-group" / "GroupGenerator.h").read_text()
    gc = (REF / "read-group" / "GroupGenerator.cpp").read_text()
    ch = (REF / "commons" / "common.h").read_text()
    header = [block(gh, "struct Relation {", ";"), block(gh, "inline Relation makeRelation("),
              line_of(gh, "static const uint32_t MERGE_SUPPORT_FLOOR"),
              block(gh, "class DisjointSet {", ";"), block(gh, "static inline void addSat16("),
              block(gh, "inline size_t getRouteRangeSize("), block(gh, "inline size_t routeOf("),
              line_of(gh, "static const size_t M_HIST_BUCKETS"), block(gh, "static inline size_t mHistBucket("),
              block(gh, "static inline size_t capFromQuantile(")]
    buffers = [block(ch, "template<typename T>\nstruct ReadBuffer {", ";"),
               block(ch, "template<typename T>\nstruct WriteBuffer {", ";")]
    methods = (definitions(gc, r"void GroupGenerator::makeGroups\(") +
               definitions(gc, r"void GroupGenerator::mergeBySupport\(") +
               definitions(gc, r"void GroupGenerator::makeGroupsPhase2\("))
    assert len(methods) == 3
    return "\n".join([
        "#include <algorithm>", "#include <cmath>", "#include <cstdint>", "#include <cstdio>", "#include <cstdlib>",
        "#include <cstring>", "#include <ctime>", "#include <functional>", "#include <iostream>", "#include <string>",
        "#include <unordered_map>", "#include <unordered_set>", "#include <vector>", "#include <omp.h>",
        "using namespace std;", *buffers, *header,
        "struct LocalParameters { int threads; };",
        "class GroupGenerator { public:",
        "  LocalParameters par; string outDir;",
        "  void makeGroups(int groupKmerThr, size_t processedReadCnt,"
        " unordered_map<uint32_t, unordered_set<uint32_t>> &groupInfo, vector<uint32_t> &queryGroupInfo);",
        "  void mergeBySupport(int coreThr, int weakThr, float supportRatio, size_t maxUnitReads, size_t processedReadCnt,"
        " unordered_map<uint32_t, unordered_set<uint32_t>> &groupInfo, vector<uint32_t> &queryGroupInfo);",
        "  void makeGroupsPhase2(int groupKmerThr, size_t processedReadCnt, const std::vector<bool>& isSingleton,"
        " unordered_map<uint32_t, unordered_set<uint32_t>>& groupInfo, vector<uint32_t>& queryGroupInfo);",
        "};", *methods, DRIVER])


# argv: <mode> <work dir> <out file>. Mode "phases": stdin "<threads> <N> <core> <weak> <E>" then E rows
# "id1 id2 weight"; out: 3 x (N + 1) uint32. Mode "cap": stdin "<cases>", per case the quantile's float
# bits and 64 counts; out: one uint64 per case. Mode "bucket": stdin "<n>" and n values; out: uint64 each.
DRIVER = r"""
int main(int argc, char **argv) {
  if (argc != 4) return 9;
  std::string mode = argv[1];
  FILE *out = fopen(argv[3], "wb");
  if (!out) return 8;
  if (mode == "cap") {
    int cases; if (scanf("%d", &cases) != 1) return 1;
    for (int c = 0; c < cases; c++) {
      unsigned bits; if (scanf("%u", &bits) != 1) return 2;
      float q; memcpy(&q, &bits, 4);
      std::vector<uint64_t> h(64);
      for (auto &x : h) { unsigned long long v; if (scanf("%llu", &v) != 1) return 3; x = v; }
      uint64_t cap = capFromQuantile(h, q);
      fwrite(&cap, 8, 1, out);
    }
  } else if (mode == "bucket") {
    int n; if (scanf("%d", &n) != 1) return 1;
    for (int i = 0; i < n; i++) {
      unsigned long long m; if (scanf("%llu", &m) != 1) return 2;
      uint64_t b = mHistBucket((size_t)m);
      fwrite(&b, 8, 1, out);
    }
  } else {
    int threads, core, weak; unsigned long long N, E;
    if (scanf("%d %llu %d %d %llu", &threads, &N, &core, &weak, &E) != 5) return 1;
    GroupGenerator g; g.par.threads = threads; g.outDir = argv[2];
    {
      std::vector<WriteBuffer<Relation>*> wb;
      for (int i = 0; i <= 2 * threads; i++)
        wb.push_back(new WriteBuffer<Relation>(g.outDir + "/relations_" + std::to_string(i) + ".bin", 4096));
      const size_t rangeSize = getRouteRangeSize((size_t)N, threads);
      for (unsigned long long e = 0; e < E; e++) {
        unsigned a, b, w; if (scanf("%u %u %u", &a, &b, &w) != 3) return 2;
        uint16_t w16 = 0; addSat16(w16, w);
        const size_t route = routeOf(a, b, threads, rangeSize);
        if (route > (size_t)(2 * threads)) return 7;  // a file the phases never read
        Relation r = makeRelation(a, b, w16);
        wb[route]->write(&r);
      }
      for (auto *w : wb) delete w;
    }
    unordered_map<uint32_t, unordered_set<uint32_t>> groupInfo;
    vector<uint32_t> q(N + 1, 0);
    g.makeGroups(core, N, groupInfo, q);
    fwrite(q.data(), 4, N + 1, out);
    g.mergeBySupport(core, weak, 0.0f, 0, N, groupInfo, q);
    fwrite(q.data(), 4, N + 1, out);
    {
      std::vector<bool> isSingleton(N + 1, false);
      for (uint32_t i = 1; i <= N; i++) { if (q[i] == 0) isSingleton[i] = true; }
      g.makeGroupsPhase2(weak, N, isSingleton, groupInfo, q);
    }
    fwrite(q.data(), 4, N + 1, out);
  }
  fclose(out);
  return 0;
}
"""

THREADS = (1, 3, 16)


def run_phases(exe, d, threads, n, edges, core, weak):
    work = pathlib.Path(d) / "work"
    if work.exists():
        for f in work.iterdir():
            f.unlink()
    work.mkdir(exist_ok=True)
    outp = pathlib.Path(d) / "maps.bin"
    inp = f"{threads} {n} {core} {weak} {len(edges)}\n" + "".join(f"{a} {b} {w}\n" for a, b, w in edges.tolist())
    subprocess.run([str(exe), "phases", str(work), str(outp)], input=inp, text=True, check=True,
                   stdout=subprocess.DEVNULL)
    return np.fromfile(outp, np.uint32).reshape(3, n + 1)


def cap_cases(rng):
    out = []
    base = [0] * 64
    for q in (0.0, 1.0, -0.5, 1.5, 0.5, 0.9, 0.99, 0.999, 0.25, 1e-9, 0.3333):
        for kind in range(6):
            h = list(base)
            if kind == 1:
                h[1] = 10
            elif kind == 2:
                h[1:6] = [1000, 500, 250, 125, 60]
            elif kind == 3:
                h[62] = 5
                h[3] = 1
            elif kind == 4:
                h[1:12] = [int(x) for x in rng.integers(0, 1 << 40, 11)]
            elif kind == 5:
                h[1], h[2] = 1, 1  # cumulative == target exactly at q = 0.5
            out.append((np.float32(q), h))
    return out


def defaults() -> dict:
    text = (REF / "workflow" / "groupGeneration.cpp").read_text()
    body = block(text, "void setGroupGenerationDefaults(")
    body = re.sub(r"//[^\n]*", "", body)
    out = {}
    for name, expr in re.findall(r"par\.(\w+)\s*=\s*([^;]+);", body):
        expr = expr.strip()
        out[name] = {"text": expr, "value": float(expr.rstrip("f")) if re.search(r"[.f]", expr) else int(expr)}
    return out


if __name__ == "__main__":
    arrays = {}
    with tempfile.TemporaryDirectory() as d:
        src = pathlib.Path(d) / "ref_groups.cpp"
        exe, exe_san = pathlib.Path(d) / "ref_groups", pathlib.Path(d) / "ref_groups_san"
        src.write_text(program())
        common = ["g++", "-std=c++17", "-fopenmp", "-Wno-unused-result", str(src)]
        subprocess.run(common + ["-O1", "-o", str(exe)], check=True)
        subprocess.run(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                 "-o", str(exe_san)], check=True)
        names = []
        for name, n, edges, core, weak in group_cases.cases():
            maps = [run_phases(exe, d, t, n, edges, core, weak) for t in THREADS]
            for m in maps[1:]:
                assert np.array_equal(m, maps[0]), f"{name}: maps differ across thread counts"
            san = run_phases(exe_san, d, 3, n, edges, core, weak)
            assert np.array_equal(san, maps[0]), f"{name}: the sanitizer build disagrees"
            arrays[f"{name}_maps"] = maps[0]
            arrays[f"{name}_edges"] = edges.astype(np.uint32)
            arrays[f"{name}_shape"] = np.array([n, core, weak], np.int64)
            names.append(name)
            print(name, n, len(edges), "groups after each phase:",
                  [int((m[1:] == np.arange(1, n + 1)).sum()) for m in maps[0]])
        arrays["names"] = np.array(names)
        arrays["threads"] = np.array(THREADS)
        arrays["threads_agree"] = np.array(True)
        arrays["sanitizer_clean"] = np.array(True)
        cc = cap_cases(np.random.default_rng(7))
        inp = f"{len(cc)}\n" + "".join(f"{int(q.view(np.uint32))} " + " ".join(map(str, h)) + "\n" for q, h in cc)
        outp = pathlib.Path(d) / "cap.bin"
        for e in (exe, exe_san):
            subprocess.run([str(e), "cap", d, str(outp)], input=inp, text=True, check=True)
        arrays["cap_quantile"] = np.array([q for q, _ in cc], np.float32)
        arrays["cap_hist"] = np.array([h for _, h in cc], np.uint64)
        arrays["cap_value"] = np.fromfile(outp, np.uint64)
        ms = list(range(0, 70)) + [2 ** k + o for k in range(7, 64, 5) for o in (-1, 0, 1)]
        subprocess.run([str(exe), "bucket", d, str(outp)], input=f"{len(ms)}\n" + " ".join(map(str, ms)) + "\n",
                       text=True, check=True)
        arrays["bucket_m"] = np.array(ms, np.uint64)
        arrays["bucket_value"] = np.fromfile(outp, np.uint64)
    np.savez_compressed(HERE / "ref_groups.npz", **arrays)
    (HERE / "group_defaults.json").write_text(json.dumps(
        {"source": "src/workflow/groupGeneration.cpp: setGroupGenerationDefaults", "defaults": defaults()}, indent=1) + "\n")
    print("wrote", HERE / "ref_groups.npz", (HERE / "ref_groups.npz").stat().st_size, "bytes")
