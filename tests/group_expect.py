"""Plain-Python restatement of the reference's read grouping, for the tests.

Pinned to the reference's own code through fixtures (tests/test_group_expect.py): the three phases
(ref_groups.npz: makeGroups, mergeBySupport, makeGroupsPhase2 run on tests/group_cases.py),
capFromQuantile and mHistBucket (ref_groups.npz), the defaults (group_defaults.json). Restated, not
pinned: thresholds() (GroupGenerator.cpp:171-192, inline in startGroupGeneration) and the clique /
weight rule edges_from_kmers() (makeSubGraph's lambda, GroupGenerator.cpp:649-701, tied to the
reference's file readers).
"""
import numpy as np


def thresholds(min_overlap_ratio, weak_band_ratio, total_kmers, reads):
    """(coreThr, weakThr) in the reference's types: float x double, then float x int + 0.5f."""
    kpr = np.float64(total_kmers) / np.float64(reads) if reads > 0 else np.float64(0.0)
    core = int(np.float64(np.float32(min_overlap_ratio)) * kpr + np.float64(0.5))
    if core < 2:
        raise ValueError(f"core threshold resolves to {core}")
    weak = int(np.float32(np.float32(weak_band_ratio) * np.float32(core)) + np.float32(0.5))
    weak = max(weak, 1)
    if weak >= core:
        weak = core - 1
    return core, weak


def m_hist_bucket(m: int) -> int:
    b = 0
    while (m >> b) > 1 and b + 1 < 64:
        b += 1
    return b


def cap_from_quantile(hist, quantile) -> int:
    q = np.float32(quantile)
    if not (q > 0) or not (q < 1):
        return 0
    total = int(sum(int(x) for x in hist))
    if total == 0:
        return 0
    target = np.float64(total) * np.float64(q)
    cum = 0
    for b, x in enumerate(hist):
        cum += int(x)
        if np.float64(cum) >= target:
            return 0 if b + 1 >= 63 else (1 << (b + 1)) - 1
    return 0


class _DisjointSet:
    def __init__(self, n):
        self.parent = list(range(n + 1))
        self.grouped = [False] * (n + 1)

    def find(self, x):
        p = self.parent
        r = x
        while p[r] != r:
            r = p[r]
        while p[x] != r:
            p[x], x = r, p[x]
        return r

    def union(self, a, b):
        self.grouped[a] = self.grouped[b] = True
        ra, rb = self.find(a), self.find(b)
        if ra != rb:
            self.parent[max(ra, rb)] = min(ra, rb)  # the root stays the component's smallest ID

    def labels(self, n, into):
        for i in range(1, n + 1):
            if self.grouped[i]:
                into[i] = self.find(i)


def phases(n_reads, edges, core_thr, weak_thr):
    """groupMap after Phase 1, 1.5 and 2: a (3, n_reads + 1) uint32 array. edges: rows (id1, id2, weight)."""
    n = n_reads
    edges = [(int(a), int(b), int(w)) for a, b, w in np.asarray(edges).reshape(-1, 3)
             if a and b and a <= n and b <= n]
    maps = np.zeros((3, n + 1), np.uint32)
    # Phase 1
    ds = _DisjointSet(n)
    for a, b, w in edges:
        if w > core_thr:
            ds.union(a, b)
    g = [0] * (n + 1)
    ds.labels(n, g)
    maps[0] = g
    # Phase 1.5 (mergeSupportRatio = 0, mergeMaxUnitReads = 0): the disjoint set goes on from Phase 1's
    unit = [g[i] if g[i] else i for i in range(n + 1)]
    support = {}
    for a, b, w in edges:
        if w <= weak_thr or w > core_thr or (g[a] == 0 and g[b] == 0):
            continue
        u, v = unit[a], unit[b]
        if u != v:
            key = (min(u, v), max(u, v))
            support[key] = support.get(key, 0) + 1
    for (u, v), c in support.items():
        if c >= 2:
            ds.union(u, v)
    g2 = [0] * (n + 1)
    ds.labels(n, g2)
    maps[1] = g2
    # Phase 2
    ds2 = _DisjointSet(n)
    for a, b, w in edges:
        if g2[a] == 0 and g2[b] == 0 and w > weak_thr:
            ds2.union(a, b)
    g3 = list(g2)
    ds2.labels(n, g3)
    maps[2] = g3
    return maps


def edges_from_kmers(values, read_ids, max_kmer_reads=1000, max_kmer_quantile=0.0):
    """makeSubGraph's rule on (k-mer value, read ID) instances: per distinct value the sorted distinct
    reads (m of them); histograms over the k-mers with m >= 2; the cap; every kept k-mer adds 1 to each
    pair (id_i < id_j) of its reads, saturating at 65535. A dict of pairs, filled for all the runs of one
    m at a time. Returns a dict: edges (E, 3) sorted by (id1, id2), skipped (value, m) sorted by value,
    runs (value, m) of every distinct value in value order, hist_kmers, hist_pairs, cap, distinct,
    kept_pair_occurrences, max_clique."""
    values = np.asarray(values, np.uint64)
    read_ids = np.asarray(read_ids, np.uint32)
    order = np.lexsort((read_ids, values))
    v, r = values[order], read_ids[order]
    if len(v):
        first = np.concatenate([[True], (v[1:] != v[:-1]) | (r[1:] != r[:-1])])
        v, r = v[first], r[first]  # a read holds a value once, whatever its frames and mates
    starts = np.concatenate([[0], np.nonzero(v[1:] != v[:-1])[0] + 1, [len(v)]]) if len(v) else np.array([0])
    run_value, run_m = v[starts[:-1]], np.diff(starts)
    hk, hp = [0] * 64, [0] * 64
    for m in run_m[run_m >= 2].tolist():
        hk[m_hist_bucket(m)] += 1
        hp[m_hist_bucket(m)] += m * (m - 1) // 2
    cap = max_kmer_reads if max_kmer_reads > 0 else cap_from_quantile(hk, max_kmer_quantile)
    over = (run_m > cap) if cap > 0 else np.zeros(len(run_m), bool)
    skipped = np.stack([run_value[over], run_m[over].astype(np.uint64)], 1) if over.any() else np.zeros((0, 2), np.uint64)
    weights, occ, max_clique = {}, 0, 0
    for m in sorted(set(run_m[(run_m >= 2) & ~over].tolist())):
        rows = np.nonzero((run_m == m) & ~over)[0]
        ids = r[starts[rows][:, None] + np.arange(m)[None, :]].astype(np.uint64)  # (runs, m), ascending per row
        a, b = np.triu_indices(m, 1)
        keys, cnt = np.unique(ids[:, a] << np.uint64(32) | ids[:, b], return_counts=True)
        for k, c in zip(keys.tolist(), cnt.tolist()):
            weights[k] = weights.get(k, 0) + c
        occ += len(rows) * (m * (m - 1) // 2)
        max_clique = max(max_clique, m * (m - 1) // 2)
    keys = np.array(sorted(weights), np.uint64)
    edges = np.zeros((len(keys), 3), np.int64)
    if len(keys):
        edges[:, 0] = keys >> np.uint64(32)
        edges[:, 1] = keys & np.uint64(0xFFFFFFFF)
        edges[:, 2] = [min(weights[k], 65535) for k in keys.tolist()]
    return {"edges": edges, "skipped": skipped, "runs": np.stack([run_value, run_m.astype(np.uint64)], 1),
            "hist_kmers": hk, "hist_pairs": hp, "cap": cap, "distinct": len(run_m), "kept_pair_occurrences": occ,
            "max_clique": max_clique}


def group_map_bytes(group_map) -> bytes:
    """saveGroupsToFile's groupMap (GroupGenerator.cpp:2083-2085)."""
    return "".join(f"{i}\t{int(g)}\n" for i, g in enumerate(group_map) if i).encode()
