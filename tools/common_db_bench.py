#!/usr/bin/env python3
"""Stage times of the common-k-mer DB build on one GPU (not bench.py: no merge condition hangs on these).

Generates a genome collection on the device (gpu_synth: species in genera of --per-genus sister species whose
genomes are --species-div-diverged copies of one genus genome, --strains strains each), builds the DB from the
device-resident sequence (dbbuild.build_common_kmer_db, device_seq) and writes mtb_common_last_ms per stage
plus k-mers/s as JSON. k-mers: the six-frame windows of the collection (6 * (L / 3 - 11) per genome of L bases);
extract_sort_kmers_per_s is what compares with tools/group_bench.py's extract + kmer_sort over its k-mers.

    python tools/common_db_bench.py --species 64 --genome-len 2000000 --strains 2 \
        --out profiles/common_db/common_db_stages.json
"""
import argparse
import json
import os
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

STAGES = ["extract", "sort", "reduce", "fold", "encode", "total"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--species", type=int, default=64)
    ap.add_argument("--genome-len", type=int, default=2000000)
    ap.add_argument("--strains", type=int, default=2)
    ap.add_argument("--per-genus", type=int, default=4)
    ap.add_argument("--species-div", type=float, default=0.05)
    ap.add_argument("--syncmer", type=int, default=1)
    ap.add_argument("--smer-len", type=int, default=5)
    ap.add_argument("--batch-genomes", type=int, default=0, help="MTB_COMMON_BATCH_GENOMES for the run (0: unset)")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "common_db" / "common_db_stages.json"))
    a = ap.parse_args()

    import torch

    from metabuli_work_amd import gpu_synth, synth
    from metabuli_work_amd.dbbuild import build_common_kmer_db, common_last_ms

    if a.batch_genomes:
        os.environ["MTB_COMMON_BATCH_GENOMES"] = str(a.batch_genomes)
    dev = torch.device("cuda:0")
    taxo = synth.make_taxonomy(a.species, a.strains, seed=7, block_species=a.species, block_size=a.per_genus)
    taxo, gen, seq, off_t, _ = gpu_synth.make_genomes_gpu(a.species, a.genome_len, a.strains, 7, dev, taxo=taxo,
                                                          per_genus=a.per_genus, species_div=a.species_div)
    torch.cuda.synchronize()
    lens = (gen.off[1:] - gen.off[:-1]).astype("int64")
    windows = int(sum(max(0, (int(n) - f % 3) // 3 - 11) for n in lens.tolist() for f in range(6)))
    runs = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        db = build_common_kmer_db(gen, taxo, None, syncmer=a.syncmer, smer_len=a.smer_len, device_seq=(seq, off_t))
        wall = time.perf_counter() - t0
        runs.append({"wall_s": wall, "ms": dict(zip(STAGES, common_last_ms()))})
    best = min(runs, key=lambda r: r["ms"]["total"])
    ms = best["ms"]
    out = {"command": "python tools/common_db_bench.py " + " ".join(sys.argv[1:]),
           "genomes": int(gen.n), "species": a.species, "bases": int(gen.off[-1]), "syncmer": a.syncmer,
           "smer_len": a.smer_len, "windows": windows, "db_kmers": int(db.n_kmers),
           "extract_sort_kmers_per_s": windows / ((ms["extract"] + ms["sort"]) * 1e-3),
           "kmers_per_s": windows / (ms["total"] * 1e-3), "best": best, "runs": runs}
    p = pathlib.Path(a.out)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"stage_ms": ms, "windows": windows, "db_kmers": out["db_kmers"],
                      "extract_sort_kmers_per_s": out["extract_sort_kmers_per_s"], "kmers_per_s": out["kmers_per_s"],
                      "wall_s": best["wall_s"]}))


if __name__ == "__main__":
    main()
