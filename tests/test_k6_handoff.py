"""K5 -> K6 hand-off: the live pack writes the run flags, the run index is built per read and per run.

Every case is a batch cut from the oracle's sorted matches (about 300 paired reads and 40 long
reads on fmt2 and fmt1): per-read sublists that keep each read's compareMatches order, with the
sequence IDs rewritten to the batch's read numbers. The oracle's assign on exactly those matches is
the reference; the device runs them
  - through the pruning K5 and the live pack (assign_chunks: the pack writes the flags),
  - through the kept stages (assign_matches on a shuffled copy: the no-copy flag producer),
  - and both again on the general paths (MTB_FORCE_GENERIC),
and every result is compared as test_stage_parity does: scores bitwise, taxID:count lists element
by element.

The shapes are the ones where the flag producer and the run index can go wrong: reads with no
(live) match at either end of the batch and in a row, one (species, frame) group of 63 / 64 / 65 /
128 / 129 matches (the pack's 64-lane round: the predecessor of a round's first match is read
directly), a group boundary exactly at a round's first lane, two reads whose boundary matches share
species and frame (the flag comes from the read change alone), groups of pm - 1 and pm matches (pm =
the fewest matches of a path-capable group, 4 on these DBs) and of 2, 3 and 4 matches, a
path-capable group as the last of the array, and long reads with a group of >= 256 matches (the
wave forms of the path search and of chooseBestTaxon).

Every case runs again with MTB_K6_LOOKAHEAD=0 (the path search's records by indexed reads, as
before the look-ahead cursor) and the two outputs must be equal; and both again with
MTB_PATHS_NOLDS=4, which takes every group through the unstaged form (small batches fit the LDS
stage otherwise, and the cursor would not run on the small groups). The run index itself has no
earlier form left to select (its per-match arrays are gone from the context): its reference is the
oracle.
"""
import os

import numpy as np
import pytest

from metabuli_work_amd import synth
from metabuli_work_amd._abi import info_frame, info_seq
from metabuli_work_amd.classifier import Classifier, LocalParameters
from tests import oracle_ctypes as oc
from tests.test_gpu_parity import compare_results

pytestmark = pytest.mark.gpu

PM = 4            # prune_min_matches(4, 9, 1): the fewest matches of a path-capable group on these DBs
BIG_GROUP = 256   # kBigGroup: groups from here on take k_match_paths_wave
SEQ_MASK = np.uint64(0x1FFFFFFF << 32)


class Pool:
    """The oracle's matches of one read set, split by read (each in compareMatches order)."""

    def __init__(self, db_dir, gen, kind):
        self.db_dir = db_dir
        self.kind = kind
        self.par = LocalParameters(seqMode=2 if kind == "paired" else 3)
        self.par.load_db_parameters(db_dir)
        self.opar = self.par.to_c()
        if kind == "paired":
            reads = synth.make_reads(gen, 300, paired=True, seed=5, short_frac=0.03, rate_n=0.002,
                                     rate_iupac=0.001, rate_lower=0.002)
        else:
            reads = synth.make_long_reads(gen, 40, n50=3000, min_len=400, seed=5)
        self.odb = oc.OracleDb(db_dir)
        okmers, self.ql1, self.ql2 = oc.extract(self.opar, reads)
        om = oc.match(self.odb, self.opar, okmers)
        seq = info_seq(om["qinfo"]).astype(np.int64)
        self.reads = [om[seq == r + 1] for r in range(reads.n)]
        self.clf = {}

    def classifier(self, generic):
        if generic not in self.clf:
            old = os.environ.get("MTB_FORCE_GENERIC")
            os.environ["MTB_FORCE_GENERIC"] = "1" if generic else "0"  # read when the context opens
            try:
                self.clf[generic] = Classifier(self.par, db_dir=self.db_dir)
            finally:
                if old is None:
                    del os.environ["MTB_FORCE_GENERIC"]
                else:
                    os.environ["MTB_FORCE_GENERIC"] = old
        return self.clf[generic]

    def close(self):
        for c in self.clf.values():
            c.close()
        self.odb.close()


_pools = {}


@pytest.fixture(scope="module")
def pools(make_db):
    def get(db_name, kind):
        if (db_name, kind) not in _pools:
            db_dir, _, gen = make_db(db_name)
            _pools[db_name, kind] = Pool(db_dir, gen, kind)
        return _pools[db_name, kind]

    yield get
    for p in _pools.values():
        p.close()
    _pools.clear()


def groups(m):
    """The (species, frame) groups of one read's sorted matches, as arrays."""
    if len(m) == 0:
        return []
    key = m["species_id"].astype(np.uint64) << np.uint64(3) | info_frame(m["qinfo"])
    cut = np.flatnonzero(key[1:] != key[:-1]) + 1
    return np.split(m, cut)


def biggest_group(pool):
    """(read, group index, group) of the read set's largest group."""
    best = None
    for r, m in enumerate(pool.reads):
        for i, g in enumerate(groups(m)):
            if best is None or len(g) > len(best[2]):
                best = (r, i, g)
    return best


def run_case(pool, parts):
    """parts: (source read, its matches for this batch) per batch read."""
    n = len(parts)
    ms = []
    for j, (_, m) in enumerate(parts):
        m = m.copy()
        m["qinfo"] = (m["qinfo"] & ~SEQ_MASK) | (np.uint64(j + 1) << np.uint64(32))
        ms.append(m)
    empty = pool.reads[0][:0]
    matches = np.ascontiguousarray(np.concatenate(ms) if ms else empty)
    counts = np.array([len(m) for m in ms], np.uint32)
    src = np.array([s for s, _ in parts], np.int64)
    ql1 = np.ascontiguousarray(pool.ql1[src])
    ql2 = np.ascontiguousarray(pool.ql2[src])
    ores, otc = oc.assign(pool.odb, pool.opar, matches, ql1, ql2)
    ql = (ql1 + ql2).astype(np.uint32)
    shuffled = matches[np.random.default_rng(0).permutation(len(matches))]

    def both(clf):
        ar = clf.assign_chunks(matches, len(matches), counts, 1, ql, n)  # pruning K5 + live pack (general: none)
        compare_results(ar.results, ar.taxcnt, ores, otc)
        br = clf.assign_matches(shuffled, ql)  # kept stages: flags without the copy
        compare_results(br.results, br.taxcnt, ores, otc)
        return ar, br

    knobs = ("MTB_K6_LOOKAHEAD", "MTB_PATHS_NOLDS")  # both read per batch
    old = {k: os.environ.pop(k, None) for k in knobs}
    try:
        for nolds in (None, "4"):
            out = []
            for look in (None, "0"):
                for k, v in zip(knobs, (look, nolds)):
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
                out.append(both(pool.classifier(False)))
            for new, parent in zip(*out):  # the look-ahead against the indexed reads
                assert new.results.tobytes() == parent.results.tobytes()
                assert new.taxcnt.tobytes() == parent.taxcnt.tobytes()
    finally:
        for k in knobs:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    both(pool.classifier(True))  # the general paths
    return ores


def _live_read(pool):
    """A read with a path-capable group (its index)."""
    for r, m in enumerate(pool.reads):
        if any(len(g) >= PM for g in groups(m)):
            return r
    raise AssertionError("no path-capable group in the read set")


def _dead(pool, r):
    """The read cut to one group of pm - 1 matches: K5 prunes all of it."""
    g = next(g for g in groups(pool.reads[r]) if len(g) >= PM)
    return (r, g[:PM - 1])


def case_whole(pool):
    return [(r, m) for r, m in enumerate(pool.reads)]


def case_no_matches(pool):
    return [(r, pool.reads[r][:0]) for r in range(5)]


def case_one_read(pool):
    r = _live_read(pool)
    return [(r, pool.reads[r])]


def case_one_dead_read(pool):
    return [_dead(pool, _live_read(pool))]


def case_empty_reads(pool):
    """Reads without any match first, last and three in a row."""
    r = _live_read(pool)
    e = (r, pool.reads[r][:0])
    a = (r, pool.reads[r])
    return [e, a, a, e, e, e, a, e]


def case_dead_reads(pool):
    """Reads whose matches are all pruned first, last and three in a row (and next to empty ones)."""
    r = _live_read(pool)
    d = _dead(pool, r)
    e = (r, pool.reads[r][:0])
    a = (r, pool.reads[r])
    return [d, a, d, d, d, a, e, d, a, d]


def case_round_sizes(pool):
    """One species and frame with 63 .. 129 matches per read."""
    r, _, g = biggest_group(pool)
    assert len(g) >= 129
    return [(r, g[:k]) for k in (63, 64, 65, 128, 129)]


def case_round_boundary(pool):
    """A group boundary at the first lane of the pack's second and third round."""
    for r, m in enumerate(pool.reads):
        gs = groups(m)
        for i in range(len(gs) - 1):
            if len(gs[i]) >= 128:
                tail = np.concatenate(gs[i + 1:])
                return [(r, np.concatenate([gs[i][:64], tail])), (r, np.concatenate([gs[i][:128], tail]))]
    raise AssertionError("no group of 128 matches followed by another")


def case_shared_boundary(pool):
    """Neighbouring reads end and begin in the same species and frame."""
    r, _, g = biggest_group(pool)
    k = min(len(g), 70)
    return [(r, g[:k]), (r, g[:k]), (r, g[:PM]), (r, g[:PM]), (r, g[:PM - 1]), (r, g[:k])]


def case_small_groups(pool):
    """Single-group reads of 2, 3, 4 (= pm - 1, pm; the path search's look-ahead sizes) and 5 matches,
    and reads whose every group is cut to those sizes in turn."""
    r, _, g = biggest_group(pool)
    parts = [(r, g[:k]) for k in (2, 3, 4, 5, 1)]
    for q, m in enumerate(pool.reads[:40]):
        gs = groups(m)
        if len(gs) >= 2:
            parts.append((q, np.concatenate([x[:2 + (i + q) % 4] for i, x in enumerate(gs)])))
    return parts


def case_last_group_capable(pool):
    """The array ends with a path-capable group."""
    r = _live_read(pool)
    gs = groups(pool.reads[r])
    i = max(i for i, g in enumerate(gs) if len(g) >= PM)
    rb, _, g = biggest_group(pool)
    return [(r, pool.reads[r]), (rb, g[:PM]), (r, np.concatenate(gs[:i + 1]))]


def case_big_group(pool):
    """Long reads with a group of >= 256 matches: the wave forms stay on the new arrays."""
    r, _, g = biggest_group(pool)
    assert len(g) >= BIG_GROUP
    other = (r + 1) % len(pool.reads)
    return [(r, pool.reads[r]), (other, pool.reads[other]), (r, g)]


PAIRED = [case_whole, case_no_matches, case_one_read, case_one_dead_read, case_empty_reads, case_dead_reads,
          case_shared_boundary, case_small_groups, case_last_group_capable]
LONG = [case_whole, case_no_matches, case_one_read, case_empty_reads, case_dead_reads, case_round_sizes,
        case_round_boundary, case_shared_boundary, case_small_groups, case_last_group_capable, case_big_group]


@pytest.mark.parametrize("db_name", ["fmt2", "fmt1"])
@pytest.mark.parametrize("kind,case", [("paired", c) for c in PAIRED] + [("long", c) for c in LONG],
                         ids=lambda x: x if isinstance(x, str) else x.__name__[5:])
def test_handoff(pools, db_name, kind, case):
    pool = pools(db_name, kind)
    parts = case(pool)
    ores = run_case(pool, parts)
    if case in (case_whole, case_one_read, case_big_group, case_round_sizes):
        assert ores["is_classified"].any()  # the case reaches the scoring, not only the empty paths
