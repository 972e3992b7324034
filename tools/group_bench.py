#!/usr/bin/env python3
"""Stage times of the read grouping on one GPU (not bench.py: no merge condition hangs on these).

Generates read pairs on the device (gpu_synth) at a coverage where k-mers are shared by several reads,
runs the device path of grouping.group_reads (add_batch with device pointers, build_edges, finish)
and writes mtb_group_stats.ms per stage plus edges/s as JSON.

    python tools/group_bench.py --pairs 1000000 --species 20 --genome-len 1000000 \
        --out profiles/r10/group_stages.json

--common-kmers N attaches a common-k-mer set of N values (half sampled from the run's own distinct k-mers,
but at most half of those, so that k-mers are left to group; the rest random; passed from the host through
set_common_kmers) and
adds the filter's four stages (mtb_group_filter_stats.ms) and its lookups per second.
"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FILTER_STAGES = ["set_load", "membership", "neighbourhood", "compaction"]
STAGES = ["extract", "kmer_sort", "run_pass", "pair_rounds", "merge_records", "phase1", "phase1_5", "phase2"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--species", type=int, default=20)
    ap.add_argument("--genome-len", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=250000)
    ap.add_argument("--pair-budget", type=int, default=0)
    ap.add_argument("--syncmer", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--common-kmers", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r10" / "group_stages.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from metabuli_work_amd import gpu_synth
    from metabuli_work_amd._abi import MTB_INPUT_DEVICE
    from metabuli_work_amd.grouping import GroupParams, ReadGrouper

    dev = torch.device("cuda:0")
    _, _, seq, off_t, _ = gpu_synth.make_genomes_gpu(a.species, a.genome_len, 1, 7, dev)
    s1, o1, s2, o2 = gpu_synth.make_reads_gpu(seq, off_t, a.pairs, 8, dev, random_frac=0.0)
    torch.cuda.synchronize()
    par = GroupParams(syncmer=a.syncmer)

    def add_batches(g):
        for b0 in range(0, a.pairs, a.batch):
            b1 = min(a.pairs, b0 + a.batch)
            offs = [(o[b0:b1 + 1] - o[b0]).contiguous() for o in (o1, o2)]
            seqs = [s[int(o[b0]):int(o[b1])].contiguous() for s, o in ((s1, o1), (s2, o2))]
            torch.cuda.synchronize()
            g.add_batch(seqs[0].data_ptr(), (offs[0].data_ptr(), b1 - b0), seqs[1].data_ptr(),
                        (offs[1].data_ptr(),), flags=MTB_INPUT_DEVICE)

    common, own_n = None, 0
    if a.common_kmers:
        with ReadGrouper(par) as g:
            add_batches(g)
            distinct = np.unique(g.kmers()[0])
        rng = np.random.default_rng(1)
        own = rng.choice(distinct, min(a.common_kmers // 2, len(distinct) // 2), replace=False)
        own_n = len(own)
        common = np.unique(np.concatenate([own, rng.integers(0, 1 << 60, a.common_kmers - own_n, dtype=np.uint64)]))
        del distinct, own
    runs = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        with ReadGrouper(par) as g:
            if common is not None:
                g.set_common_kmers(common)
            add_batches(g)
            fst = g.filter_stats() if common is not None else None
            g.build_edges(a.pair_budget)
            gm, st = g.finish()
        wall = time.perf_counter() - t0
        ms = dict(zip(STAGES, st["ms"]))
        edge_ms = sum(ms[k] for k in ("kmer_sort", "run_pass", "pair_rounds", "merge_records"))
        runs.append({"wall_s": wall, "ms": ms, "edges_per_s": st["edges"] / (edge_ms * 1e-3) if edge_ms else 0.0,
                     "pair_occurrences_per_s": st["kept_pair_occurrences"] / (edge_ms * 1e-3) if edge_ms else 0.0})
        if fst is not None:
            fms = dict(zip(FILTER_STAGES, fst["ms"]))
            runs[-1]["filter_ms"] = fms
            runs[-1]["lookups_per_s"] = fst["extracted"] / (fms["membership"] * 1e-3) if fms["membership"] else 0.0
    best = min(runs, key=lambda r: sum(r["ms"].values()))
    out = {"command": "python tools/group_bench.py " + " ".join(sys.argv[1:]),
           "pairs": a.pairs, "species": a.species, "genome_len": a.genome_len, "syncmer": a.syncmer,
           "reads": st["reads"], "kmers": st["kmers"], "distinct_kmers": st["distinct_kmers"],
           "skipped_kmers": st["skipped_kmers"], "kept_pair_occurrences": st["kept_pair_occurrences"],
           "edges": st["edges"], "rounds": st["rounds"], "cap": st["cap"], "core_thr": st["core_thr"],
           "weak_thr": st["weak_thr"], "groups_after": st["groups_after"], "grouped_after": st["grouped_after"],
           "best": best, "runs": runs}
    if common is not None:
        out["filter"] = {k: fst[k] for k in ("extracted", "db_values", "hit", "removed", "kept")}
        out["filter"]["own_values"] = own_n
    p = pathlib.Path(a.out)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"stage_ms": best["ms"], "filter_ms": best.get("filter_ms"), "lookups_per_s": best.get("lookups_per_s"),
                      "edges_per_s": best["edges_per_s"], "edges": st["edges"],
                      "kmers": st["kmers"], "wall_s": best["wall_s"]}))


if __name__ == "__main__":
    main()
