"""Designed edge lists for the three grouping phases (tests/test_group_expect.py on the CPU,
tests/test_group_gpu.py on the device; tests/golden/make_ref_groups.py runs the reference's own
makeGroups / mergeBySupport / makeGroupsPhase2 on them).

A case is (name, n_reads, edges, core_thr, weak_thr); edges is an (E, 3) int64 array of
(id1, id2, weight) with id1 < id2. Thresholds are given to the phases directly; params_for() turns
them into parameters from which the library's threshold arithmetic yields exactly those values.
Read counts are multiples of 48 (or 1): the reference routes an edge to relations_{T + id1 / (N / T)}
when both IDs fall in one range, and reads files 0 .. 2T only, so with N no multiple of the thread
count T (1, 3 and 16 here) it would never read the last range's edges.
"""
import numpy as np

CORE, WEAK = 15, 5


def _e(rows):
    a = np.array(rows, np.int64).reshape(-1, 3)
    lo, hi = np.minimum(a[:, 0], a[:, 1]), np.maximum(a[:, 0], a[:, 1])
    a[:, 0], a[:, 1] = lo, hi
    return a


def _clique(ids, w):
    return [(a, b, w) for i, a in enumerate(ids) for b in ids[i + 1:]]


def cases():
    rng = np.random.default_rng(20261020)
    out = []
    # a chain of 5,000 reads, edge i -- i + 1 above core, in shuffled order: a long diameter
    perm = rng.permutation(5000) + 1  # the chain visits the reads in a random order of IDs too
    chain = np.stack([perm[:-1], perm[1:], np.full(4999, CORE + 1)], 1)
    out.append(("chain_shuffled_ids", 5040, _e(chain[rng.permutation(4999)]), CORE, WEAK))
    straight = np.stack([np.arange(1, 5000), np.arange(2, 5001), np.full(4999, CORE + 1)], 1)
    out.append(("chain_ascending_ids", 5040, _e(straight[rng.permutation(4999)]), CORE, WEAK))
    # a star whose centre has the largest ID
    out.append(("star_centre_largest", 96, _e([(i, 96, 40) for i in range(1, 96, 2)]), CORE, WEAK))
    # two components and one edge between them: exactly coreThr (a weak link, not joined), coreThr + 1 (joined)
    two = _clique([1, 2, 3], CORE + 3) + _clique([10, 11, 12], CORE + 3)
    out.append(("bridge_at_core", 48, _e(two + [(3, 10, CORE)]), CORE, WEAK))
    out.append(("bridge_above_core", 48, _e(two + [(3, 10, CORE + 1)]), CORE, WEAK))
    # weights exactly weakThr and weakThr + 1 between singletons
    out.append(("weak_boundary", 48, _e([(20, 21, WEAK), (22, 23, WEAK + 1), (24, 25, CORE), (26, 27, CORE + 1)]),
                CORE, WEAK))
    # unit pairs with 1 and with 2 weak links
    grp = _clique([1, 2], 30) + _clique([3, 4], 30) + _clique([5, 6], 30)
    out.append(("support_one_and_two", 48, _e(grp + [(1, 3, 10), (2, 4, 10), (4, 5, 10)]), CORE, WEAK))
    # two weak links from one singleton to one group; a third read weakly linked to that singleton only:
    # Phase 1.5 groups the singleton, so Phase 2 may not use it
    out.append(("singleton_joins_group", 48,
                _e(_clique([1, 2, 3], 30) + [(1, 7, 8), (2, 7, 8), (7, 20, 9), (20, 21, 9)]), CORE, WEAK))
    # a weak singleton-singleton pair: Phase 1.5 skips it, Phase 2 joins it
    out.append(("weak_singletons", 48, _e([(8, 9, 10), (9, 30, 6), (31, 32, WEAK)]), CORE, WEAK))
    # a merge that changes a group's smallest ID
    out.append(("merge_lowers_label", 48, _e(_clique([5, 6, 9], 30) + [(2, 5, 9), (2, 6, 9)]), CORE, WEAK))
    out.append(("merge_two_groups_lowers_label", 48,
                _e(_clique([40, 41], 30) + _clique([3, 44], 30) + [(3, 40, 6), (41, 44, 15)]), CORE, WEAK))
    # a weight of 65535, and thresholds near the top of the range
    out.append(("weight_65535", 48, _e([(1, 2, 65535), (2, 3, 65534), (4, 5, 65533)]), 65534, 65533))
    out.append(("weight_65535_default_thr", 48, _e([(1, 2, 65535), (3, 4, 1)]), CORE, WEAK))
    # isolated reads only; one read
    out.append(("no_edges", 48, _e([]), CORE, WEAK))
    out.append(("one_read", 1, _e([]), CORE, WEAK))
    # a chain of weak merges: A-B and B-C supported, so A, B and C end in one component
    tri = _clique([10, 11], 30) + _clique([20, 21], 30) + _clique([30, 31], 30)
    out.append(("support_chain", 48, _e(tri + [(10, 20, 7), (11, 21, 7), (20, 30, 7), (21, 31, 15)]), CORE, WEAK))
    # random graphs over several blocks of edges, every weight class
    for n, m, seed in ((2400, 3000, 1), (4800, 40000, 2), (960, 60000, 3)):
        r = np.random.default_rng(seed)
        a, b = r.integers(1, n + 1, m), r.integers(1, n + 1, m)
        keep = a != b
        pairs = np.unique(np.stack([np.minimum(a, b)[keep], np.maximum(a, b)[keep]], 1), axis=0)
        hi = 60 if seed == 3 else 22  # the dense one: mostly below weak, so that the phases leave structure
        w = r.integers(1, hi, len(pairs))
        if seed == 3:
            w = np.where(r.random(len(pairs)) < 0.97, r.integers(1, WEAK + 1, len(pairs)), w)
        edges = np.concatenate([pairs, w[:, None]], 1)
        out.append((f"random_{n}_{m}", n, edges[r.permutation(len(edges))], CORE, WEAK))
    return out


def params_for(core_thr: int, weak_thr: int, n_reads: int):
    """(min_overlap_ratio, weak_band_ratio, total_kmers) from which GroupGenerator.cpp:171-192's
    arithmetic gives core_thr and weak_thr: k-mers per read = core_thr exactly at ratio 1."""
    return 1.0, float(np.float32(weak_thr) / np.float32(core_thr)), core_thr * n_reads
