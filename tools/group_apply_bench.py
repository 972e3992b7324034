#!/usr/bin/env python3
"""Stage times of the group application on one GPU (not bench.py: no merge condition hangs on these).

Generates a group map and labels (no reads needed), runs grouping.apply_groups_arrays on device-resident
tensors and writes mtb_group_apply_stats.ms per stage as JSON.

    python tools/group_apply_bench.py --reads 1000000 10000000 --out profiles/group_apply/group_apply_stages.json

The generated input, per read count n: a synth taxonomy of --species species with two strains each;
80 % of the reads are grouped, group sizes drawn from a geometric distribution of mean --group-size (a
group's ID is its smallest read ID, its members scattered over the whole run); every group has a home
species: 70 % of its members carry it (half of those one of its strains), 10 % a random other species,
20 % are unclassified; scores are uniform in [0, 1); weight mode 1, min_vote_score 0.15.
"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

STAGES = ["keys_sort", "label_sums", "group_choice", "apply"]


def generate(n, taxo, group_size, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    species = np.array([t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "species"], np.int32)
    strain_of = {int(p): [] for p in species.tolist()}
    for t, p in zip(taxo.taxid.tolist(), taxo.parent.tolist()):
        if p in strain_of and t != p:
            strain_of[p].append(t)
    strains = np.array([strain_of[int(s)][0] if strain_of[int(s)] else int(s) for s in species], np.int32)
    grouped = int(0.8 * n)
    sizes = rng.geometric(1.0 / group_size, max(1, 2 * grouped // group_size + 16))
    sizes = sizes[np.cumsum(sizes) <= grouped]
    member_group = np.repeat(np.arange(len(sizes)), sizes)
    reads = rng.permutation(n)[:len(member_group)] + 1
    gid = np.full(len(sizes), n + 1, np.int64)
    np.minimum.at(gid, member_group, reads)
    gm = np.zeros(n + 1, np.uint32)
    gm[reads] = gid[member_group]
    home = rng.integers(0, len(species), len(sizes))
    tax = np.zeros(n, np.int32)
    u = rng.random(n)
    sp = rng.integers(0, len(species), n)
    sp[reads - 1] = np.where(rng.random(len(reads)) < 0.875, home[member_group], sp[reads - 1])
    tax[:] = np.where(u < 0.2, 0, np.where(u < 0.6, species[sp], strains[sp]))
    score = rng.random(n).astype(np.float32)
    return gm, tax, score, len(sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--species", type=int, default=2000)
    ap.add_argument("--group-size", type=int, default=12)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "group_apply" / "group_apply_stages.json"))
    a = ap.parse_args()

    import torch  # before the library is loaded

    from metabuli_work_amd import synth
    from metabuli_work_amd.grouping import ApplyParams, apply_groups_arrays

    taxo = synth.make_taxonomy(a.species, 2, seed=5)
    par = ApplyParams.defaults()
    out = {"command": "python tools/group_apply_bench.py " + " ".join(sys.argv[1:]), "species": a.species,
           "group_size": a.group_size, "weight_mode": par.weight_mode, "min_vote_score": par.min_vote_score, "sizes": []}
    for n in a.reads:
        gm, tax, score, n_groups = generate(n, taxo, a.group_size, 3)
        dgm = torch.from_numpy(gm.view("int32")).cuda()
        dtax, dscore = torch.from_numpy(tax).cuda(), torch.from_numpy(score).cuda()
        runs = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            *_, st = apply_groups_arrays(dgm, dtax, dscore, taxo, par)
            runs.append({"wall_s": time.perf_counter() - t0, "ms": dict(zip(STAGES, st["ms"]))})
        best = min(runs, key=lambda r: sum(r["ms"].values()))
        row = {"reads": n, "generated_groups": n_groups, "groups": st["groups"], "labels": st["labels"],
               "voting_reads": st["voting_reads"], "groups_with_rep": st["groups_with_rep"], "applied": st["applied"],
               "best": best, "runs": runs}
        out["sizes"].append(row)
        print(json.dumps({"reads": n, "groups": st["groups"], "stage_ms": best["ms"],
                          "device_ms": sum(best["ms"].values()), "wall_s": best["wall_s"]}))
    p = pathlib.Path(a.out)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
