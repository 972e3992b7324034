"""What tests/golden/ref_assign.npz holds (shared by tests/test_ref_assign.py and the fixture's generator,
tests/golden/make_ref_assign.py): loading it, the `wide` DB, and the count of the branches and shapes
it covers, recomputed from its stored inputs and outputs."""
import pathlib
import struct

import numpy as np

from metabuli_work_amd._abi import MATCH_DTYPE, default_params, info_frame, info_pos, info_seq

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
DBS = ["fmt2", "fmt1", "fmt2_syncmer", "fmt2_acc"]
BLANK = "fmt2_acc_blank"
# A DB of its own, not one of conftest's: genera enough for species under Eukaryota (make_taxonomy puts
# the last n_genera // 8 genera there) and one species with 320 further strains, so that one read's
# taxCnt can hold more taxa than K6's LDS hashes (kGroupHash 64, kTcHash 256).
WIDE = "wide"
WIDE_CONFIG = dict(kmer_format=2, n_species=16, strains=2, n_genera=8, genome_len=16000, extra_strains=320)


def wide_taxonomy_and_genomes():
    """The `wide` taxonomy (the genomes come from the taxonomy before the extra strains are added: the
    extra strains hold no genome, they are targets of constructed matches only)."""
    from metabuli_work_amd import synth
    w = WIDE_CONFIG
    taxo = synth.make_taxonomy(w["n_species"], w["strains"], seed=11, n_genera=w["n_genera"])
    gen = synth.make_genomes(taxo, genome_len=w["genome_len"], seed=12)
    sp = int(taxo.taxid[taxo.rank.index("species")])
    nxt = int(taxo.taxid.max()) + 1
    extra = list(range(nxt, nxt + w["extra_strains"]))
    taxo = synth.Taxonomy(np.concatenate([taxo.taxid, np.array(extra, np.int32)]),
                          np.concatenate([taxo.parent, np.full(len(extra), sp, np.int32)]),
                          taxo.rank + ["no rank"] * len(extra), taxo.name + [f"no rank_{t}" for t in extra])
    return taxo, gen


def build_wide_db(out_dir):
    """Builds the `wide` DB through the oracle's IndexCreator restatement; returns its taxonomy."""
    from tests import oracle_ctypes as oc
    taxo, gen = wide_taxonomy_and_genomes()
    oc.build_db(out_dir, default_params(kmer_format=WIDE_CONFIG["kmer_format"], syncmer=0, smer_len=5), taxo, gen)
    return taxo

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN / "ref_assign.npz"))
    return _golden


def fl(bits) -> float:
    return struct.unpack("<f", struct.pack("<I", int(bits)))[0]


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens).astype(np.int64))])


def matches_of(g, db):
    m = np.zeros(len(g[f"{db}_m_ham"]), MATCH_DTYPE)
    m["qinfo"] = g[f"{db}_m_qinfo"]
    m["target_id"] = g[f"{db}_m_target"]
    m["species_id"] = g[f"{db}_m_species"]
    m["dna_encoding"] = g[f"{db}_m_dna"]
    m["right_end_hamming"] = g[f"{db}_m_reh"]
    m["hamming"] = g[f"{db}_m_ham"]
    return m


def params_of(g, db):
    """One dict per parameter set (accessionLevel is the effective one, after db.parameters)."""
    cols = g["param_cols"].tolist()
    return [dict(zip(cols, (int(x) for x in row))) for row in g[f"{db}_params"]]


def c_params(p):
    return default_params(seq_mode=p["seqMode"], kmer_format=p["kmerFormat"], syncmer=p["syncmer"], smer_len=p["smerLen"],
                          min_score=fl(p["minScoreBits"]), min_sp_score=fl(p["minSpScoreBits"]),
                          min_cons_cnt=p["minConsCnt"], min_cons_cnt_euk=p["minConsCntEuk"],
                          tie_ratio=fl(p["tieRatioBits"]), accession_level=p["accessionLevel"], em=p["em"])


# ---------------------------------------------------------------------------------------------------
# which branches and shapes the fixture holds, recomputed from its inputs and outputs
def _consecutive(fmt, fwd, cur, nxt, s):
    a, b = (cur, nxt) if fwd else (nxt, cur)
    mask = (1 << (24 - 3 * s)) - 1
    return (a & mask) == (b >> (3 * s)) if fmt == 2 else (a >> (3 * s)) == (b & mask)


def _match_score(reh):
    return sum(3.0 if (reh >> (2 * i)) & 3 == 0 else 2.0 - 0.5 * ((reh >> (2 * i)) & 3) for i in range(8))


def _small_group_paths(fmt, fwd, pos, dna, reh, max_shift, min_depth, last_wins):
    """The paths a group of a few matches yields (getMatchPaths' loop in small), with the first or the
    last of tied predecessors winning: only to count the groups where that choice shows."""
    n = len(pos)
    path = [(int(pos[i]), _match_score(int(reh[i])), 1) for i in range(n)]
    conn = [False] * n
    cuts = [0] + [i for i in range(1, n) if pos[i] != pos[i - 1]] + [n]
    out = []
    for b in range(len(cuts) - 2):
        c0, c1, c2 = cuts[b], cuts[b + 1], cuts[b + 2]
        shift = int(pos[c1] - pos[c0]) // 3
        if 1 <= shift <= max_shift:
            for j in range(c1, c2):
                best, bs = None, 0.0
                for i in range(c0, c1):
                    if _consecutive(fmt, fwd, int(dna[i]), int(dna[j]), shift):
                        conn[i] = True
                        if path[i][1] > bs or (last_wins and path[i][1] >= bs):
                            best, bs = i, path[i][1]
                if best is not None:
                    inc = sum(3.0 if (int(reh[j]) >> (2 * k)) & 3 == 0 else 2.0 - 0.5 * ((int(reh[j]) >> (2 * k)) & 3)
                              for k in range(shift))
                    path[j] = (path[best][0], path[best][1] + inc, path[best][2] + shift)
        out += [path[i] for i in range(c0, c1) if not conn[i] and path[i][2] >= min_depth]
        if c2 == n:
            out += [path[i] for i in range(c1, c2) if path[i][2] >= min_depth]
    return sorted(out)


def _db_shapes(g, db, c):
    par = params_of(g, db)
    fmt, syn = par[0]["kmerFormat"], par[0]["syncmer"]
    max_shift = 8 - par[0]["smerLen"] if syn else 1
    dna_shift = 3 * max_shift if syn else 3
    euk = int(g[f"{db}_euk"])
    parent = dict(zip(g[f"{db}_tax_id"].tolist(), g[f"{db}_tax_parent"].tolist()))
    rank = dict(zip(g[f"{db}_tax_id"].tolist(), (g["rank_names"][i] for i in g[f"{db}_tax_rank"])))
    has_kids = set(parent.values())
    tag = g[f"{db}_tag"].tolist()  # the generator's case names: the proxies below also key on them

    def under_euk(t):
        while t != euk and parent[t] != t:
            t = parent[t]
        return t == euk
    m = matches_of(g, db)
    seq = info_seq(m["qinfo"]).astype(np.int64)
    frame = info_frame(m["qinfo"]).astype(np.int64)
    pos = info_pos(m["qinfo"]).astype(np.int64)
    ql = (g[f"{db}_ql1"].astype(np.int64) + g[f"{db}_ql2"])
    n_reads = len(ql)
    cnt = np.bincount(seq - 1, minlength=n_reads)
    start = _offsets(cnt)
    out = {k: {x: g[f"{db}_p{k}_{x}"] for x in ("is_classified", "classification", "score_bits", "tc_len", "tc")}
           for k in range(len(par))}
    tc_off = {k: _offsets(out[k]["tc_len"]) for k in out}

    def add(key, n=1):
        c[key] = c.get(key, 0) + int(n)

    def isc0_of(r):
        return int(out[0]["is_classified"][r])

    def tc_of(k, r):
        return out[k]["tc"][tc_off[k][r]:tc_off[k][r + 1]]

    # reads with no match
    e = cnt == 0
    add("empty_first", e[0])
    add("empty_last", e[-1])
    add("empty_three_in_a_row", np.any(e[:-2] & e[1:-1] & e[2:]))
    s2 = {k: (g[f"{db}_p{k}_s2_len"], g[f"{db}_p{k}_s2"]) for k in range(len(par)) if par[k]["em"]}
    for k, (ln, lst) in s2.items():
        off = _offsets(ln)
        for r in range(n_reads):
            if ln[r] == 0:
                continue
            sc = np.sqrt(lst[off[r]:off[r + 1], 1].astype(np.uint32).view(np.float32).astype(np.float64))
            assert int(g[f"{db}_p{k}_top"][r]) == int(lst[off[r], 0])
            ratio = np.sort(sc / sc.max())[::-1]
            within = int((ratio >= 0.9501).sum())
            if np.any(np.abs(ratio - 0.95) < 1e-4):
                add("tie_ratio_edge")
            elif within == 2:
                add("tie_two_species")
            elif within >= 3:
                add("tie_three_species")
            elif within == 1 and np.any((ratio < 0.9499) & (ratio >= 0.90)):
                add("tie_one_just_outside")

    for r in range(n_reads):
        if cnt[r] == 0:
            continue
        lo, hi = start[r], start[r + 1]
        if db == "fmt2":
            for n in (512, 513, 2048, 2049, 8193):
                add(f"read_{n}_matches", cnt[r] == n)
            for n in (255, 257):  # live matches: these reads (tag group255 / group257) are one group, all of it live
                add(f"read_{n}_matches", cnt[r] == n and tag[r] == f"group{n}")
        if db == WIDE:
            for n in (64, 65, 256, 257):  # distinct taxa of the read's taxCnt, as the reference returned it
                add(f"read_{n}_taxa", isc0_of(r) and out[0]["tc_len"][r] == n)
        sp_r, fr_r, pos_r = m["species_id"][lo:hi].astype(np.int64), frame[lo:hi], pos[lo:hi]
        key = sp_r * 8 + fr_r
        cuts = np.flatnonzero(key[1:] != key[:-1]) + 1
        bounds = np.concatenate([[0], cuts, [hi - lo]])
        species_set = set(sp_r.tolist())
        cls0, isc0 = int(out[0]["classification"][r]), int(out[0]["is_classified"][r])
        paths_per_species = {}
        best_depth = {}
        for a, b in zip(bounds[:-1], bounds[1:]):
            n = b - a
            sp, f = int(sp_r[a]), int(fr_r[a])
            if n == 1:
                add("group_of_1")
                continue
            add("group_of_2", n == 2)
            add(f"frame{f}_group")
            if db == "fmt2":
                for k in (255, 256, 257, 1023, 1025):
                    add(f"group_of_{k}", n == k)
            p = pos_r[a:b]
            if p[0] == p[-1]:
                add("group_at_one_position")
                continue
            pc = np.flatnonzero(p[1:] != p[:-1]) + 1
            pb = np.concatenate([[0], pc, [n]])
            depth, first = 1, True
            min_depth = par[0]["minConsCntEuk"] if under_euk(sp) else par[0]["minConsCnt"]
            if n <= 8:
                sl = slice(lo + a, lo + b)
                both = [_small_group_paths(fmt, f < 3, p, m["dna_encoding"][sl], m["right_end_hamming"][sl], max_shift,
                                           min_depth, lw) for lw in (False, True)]
                add("tied_predecessors_decide", both[0] != both[1])
            for i in range(len(pb) - 2):
                c0, c1, c2 = pb[i], pb[i + 1], pb[i + 2]
                step = int(p[c1] - p[c0])
                shift = step // 3
                add("step_not_multiple_of_3", step % 3 != 0 and shift >= 1)
                add("step_under_3", shift == 0)
                if syn:
                    add(f"syncmer_shift_{min(shift, 4)}", 1 <= shift <= 4)
                else:
                    add("shift_2_not_syncmer", shift == 2)
                ok = 1 <= shift <= max_shift
                k0, k1 = c1 - c0, c2 - c1
                if ok and k0 == k1 and 2 <= k0 <= 6:
                    add(f"step_{k0}_candidates_both_sides")
                if ok and first and k0 >= 2:  # first step of the group: a path's score is its match's
                    for j in range(c1, c2):
                        sc = [_match_score(int(m["right_end_hamming"][lo + a + i0])) for i0 in range(c0, c1)
                              if _consecutive(fmt, f < 3, int(m["dna_encoding"][lo + a + i0]),
                                              int(m["dna_encoding"][lo + a + j]), shift)]
                        if len(sc) >= 2 and sc.count(max(sc)) >= 2:
                            add("tied_predecessors")
                            break
                first = False
                if ok:
                    depth += shift
                else:
                    if depth >= min_depth:
                        paths_per_species[sp] = paths_per_species.get(sp, 0) + 1
                    best_depth[sp] = max(best_depth.get(sp, 0), depth)
                    depth = 1
            if depth >= min_depth:
                paths_per_species[sp] = paths_per_species.get(sp, 0) + 1
            best_depth[sp] = max(best_depth.get(sp, 0), depth)
        if len(species_set) == 1:
            # d is the depth of the longest run of linked positions: the best path's depth only where
            # every candidate is consecutive, as in the generator's perfect single chains (tags
            # euk_depth<d>, eukspecies_depth<d>, bact_depth<d>), so these counters key on the tag too
            sp = next(iter(species_set))
            d = best_depth.get(sp, 0)
            if sp == euk and tag[r] == f"euk_depth{d}":
                add("euk_depth_4_to_8_unclassified", 4 <= d <= 8 and not isc0)
                add("euk_depth_9_classified", d == 9 and isc0)
            elif under_euk(sp) and tag[r] == f"eukspecies_depth{d}":
                assert rank[sp] == "species" and sp != euk
                add("wide_euk_species_depth_4_to_8_unclassified", 4 <= d <= 8 and not isc0)
                add("wide_euk_species_depth_9_classified", d == 9 and isc0)
            elif tag[r] == f"bact_depth{d}":
                add("bacteria_depth_3_unclassified", d == 3 and not isc0)
                add("bacteria_depth_4_classified", d == 4 and isc0)
            if db == "fmt2":
                for k in (23, 24, 25):
                    add(f"species_with_{k}_paths", paths_per_species.get(sp, 0) == k)
            quot = len(np.unique(pos_r // dna_shift))
            if db == "fmt2":
                add("paired_read_over_128_quotients", quot > 128 and g[f"{db}_ql2"][r] > 0)
                add("long_read_over_4096_quotients", quot > 4096)
        sc0 = fl(out[0]["score_bits"][r])
        # a perfect chain that ends past the read length scores above 1.0 before the clamp (tag clamp)
        add("score_clamped_to_1", sc0 == 1.0 and pos_r.max() + 24 > ql[r] and tag[r] == "clamp")
        add("unclassified_score_0", not isc0 and out[0]["score_bits"][r] == 0)
        # the non-zero minScore / minSpScore set
        k2 = next(k for k in range(len(par)) if par[k]["minSpScoreBits"] != 0)
        isc2, tl2 = int(out[k2]["is_classified"][r]), int(out[k2]["tc_len"][r])
        add("unclassified_by_min_score", isc0 and not isc2)
        add("min_score_drops_a_tied_species", isc0 and out[0]["tc_len"][r] == 0 and isc2 and tl2 > 0)
        if isc2 and tl2 > 0 and fl(out[k2]["score_bits"][r]) < fl(par[k2]["minSpScoreBits"]):
            assert rank[int(out[k2]["classification"][r])] == "genus"
            add("parent_of_species_branch")
        # filterRedundantMatches and BFS, from the taxCnt list of the default set
        tc = tc_of(0, r)
        if isc0 and len(tc):
            targets = set(m["target_id"][lo:hi].tolist())
            add("taxcnt_key_is_an_lca", any(int(t) not in targets for t in tc[:, 0]))
            if len(species_set) == 1:
                seen = {}
                lower = False
                for i in range(lo, hi):
                    q = int(pos[i]) // dna_shift
                    h = int(m["hamming"][i])
                    lower |= q in seen and h < seen[q]
                    seen[q] = min(h, seen.get(q, 255))
                add("lower_hamming_second", lower)
                sp = next(iter(species_set))
                kid = {}
                for t, n in tc.tolist():
                    while t != sp and parent[t] != sp:
                        t = parent[t]
                    if t != sp:
                        kid[t] = kid.get(t, 0) + n
                for k in (0, 1):
                    thr = (int(ql[r]) - 1) // (100 if par[k]["seqMode"] in (1, 2) else 1000)
                    ck, isk = int(out[k]["classification"][r]), int(out[k]["is_classified"][r])
                    if not isk or not kid or thr == 0:
                        continue
                    top = sorted(kid.values())[::-1]
                    add(f"bfs_best_child_at_threshold_seqmode{par[k]['seqMode']}", top[0] == thr and ck == sp)
                    add("bfs_down_to_a_leaf", ck not in has_kids and ck != sp)
                    if k == 0:
                        add("bfs_two_tied_children_stays", len(top) > 1 and top[0] == top[1] > thr and ck == sp)
        if par[0]["accessionLevel"] == 2:
            c0, c1 = cls0, int(out[1]["classification"][r])
            if isc0 and c1 != c0 and c1 in rank:
                add("accession_level_1_reaches_accession", rank[c1] == "accession")
                add("accession_leaf_removed_at_level_2", rank[c1] == "accession" and c0 == parent[c1])
                add("blank_rank_leaf_removed_at_level_2", rank[parent[c1]] == "" and rank[c0] == "species")


def _dna_shapes(g, c):
    import json
    look = json.loads((GOLDEN / "hamming_tables.json").read_text())["hammingLookup"]
    off = _offsets(g["dna_n"])
    koff = _offsets(g["dna_k"])
    for i in range(len(g["dna_n"])):
        q = int(g["dna_query"][i])
        tg = [int(t) for t in g["dna_targets"][off[i]:off[i + 1]]]
        sums = [sum(look[(q >> (3 * j)) & 7][(t >> (3 * j)) & 7] for j in range(8)) for t in tg]
        sel = g["dna_sel"][koff[i]:koff[i + 1]]
        assert all(t >> 24 == q >> 24 for t in tg)  # equal in AA, differing only in DNA
        mn = min(sums)
        key = f"dna_min_hamming_{mn}" if mn < 4 else "dna_min_hamming_4_or_more"
        c[key] = c.get(key, 0) + 1
        for k, on in ((f"dna_fmt{g['dna_fmt'][i]}_frame{g['dna_frame'][i]}", True), ("dna_list_of_1", len(tg) == 1),
                      ("dna_list_of_40", len(tg) == 40), ("dna_list_at_one_distance", len(tg) > 1 and len(set(sums)) == 1),
                      ("dna_some_rejected", len(sel) < len(tg)),
                      ("dna_cap_7_decides", 2 * mn > 7 and 7 in sums and max(sums) > 7)):
            c[k] = c.get(k, 0) + int(on)


def coverage_table(g):
    """Shape -> how many times the fixture holds it: for the shapes every k-mer format must hold, the
    fewest over the DBs."""
    per_db = {}
    for db in DBS + [BLANK, WIDE]:
        per_db[db] = {}
        _db_shapes(g, db, per_db[db])
    fmt2_only = ("read_", "species_with_", "paired_read_over", "long_read_over") + tuple(
        f"group_of_{n}" for n in (255, 256, 257, 1023, 1025))
    table = {}
    for k in sorted({k for d in per_db for k in per_db[d]}):
        if k.endswith("_taxa"):
            table[k] = per_db[WIDE].get(k, 0)
        elif k.startswith(fmt2_only):
            table[k] = per_db["fmt2"].get(k, 0)
        elif k.startswith("syncmer_shift"):
            table[k] = per_db["fmt2_syncmer"].get(k, 0)
        elif k == "shift_2_not_syncmer":
            table[k] = min(per_db[d].get(k, 0) for d in DBS if d != "fmt2_syncmer")
        elif k.startswith("accession_"):
            table[k] = per_db["fmt2_acc"].get(k, 0)
        elif k.startswith("wide_"):
            table[k] = per_db[WIDE].get(k, 0)
        elif k.startswith("blank_"):
            table[k] = per_db[BLANK].get(k, 0)
        elif k == "tie_ratio_edge":
            table[k] = sum(per_db[d].get(k, 0) for d in DBS)
        else:
            table[k] = min(per_db[d].get(k, 0) for d in DBS)
    _dna_shapes(g, table)
    return table


EXPECTED_SHAPES = (
    [f"frame{f}_group" for f in range(6)] + ["group_of_1", "group_of_2", "group_at_one_position", "tied_predecessors",
                                                   "tied_predecessors_decide"] +
    [f"step_{k}_candidates_both_sides" for k in range(2, 7)] + ["step_not_multiple_of_3", "step_under_3"] +
    [f"syncmer_shift_{s}" for s in (1, 2, 3, 4)] + ["shift_2_not_syncmer", "euk_depth_4_to_8_unclassified",
     "euk_depth_9_classified", "bacteria_depth_3_unclassified", "bacteria_depth_4_classified", "score_clamped_to_1",
     "unclassified_by_min_score", "min_score_drops_a_tied_species", "tie_two_species", "tie_three_species",
     "tie_one_just_outside", "parent_of_species_branch", "unclassified_score_0", "taxcnt_key_is_an_lca",
     "lower_hamming_second", "bfs_down_to_a_leaf", "bfs_two_tied_children_stays",
     "bfs_best_child_at_threshold_seqmode2", "bfs_best_child_at_threshold_seqmode3",
     "accession_level_1_reaches_accession", "accession_leaf_removed_at_level_2",
     "blank_rank_leaf_removed_at_level_2", "wide_euk_species_depth_4_to_8_unclassified",
     "wide_euk_species_depth_9_classified", "read_64_taxa", "read_65_taxa", "read_256_taxa", "read_257_taxa"] +
    [f"group_of_{n}" for n in (255, 256, 257, 1023, 1025)] +
    [f"read_{n}_matches" for n in (255, 257, 512, 513, 2048, 2049, 8193)] +
    ["paired_read_over_128_quotients", "long_read_over_4096_quotients"] +
    [f"species_with_{k}_paths" for k in (23, 24, 25)] +
    ["empty_first", "empty_last", "empty_three_in_a_row"] +
    [f"dna_fmt{f}_frame{fr}" for f in (1, 2) for fr in range(6)] +
    [f"dna_min_hamming_{k}" for k in range(4)] + ["dna_min_hamming_4_or_more", "dna_list_of_1", "dna_list_of_40",
     "dna_list_at_one_distance", "dna_some_rejected", "dna_cap_7_decides"])
