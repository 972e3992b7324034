"""mtb_em (k_em_estep, k_em_slices, k_em_mstep, k_em_delta, k_em_reclassify, k_species_kmers) on designed
mappings. No read is classified here: the mappings are made in numpy and handed to Classifier.em.

The DB is this file's own: 300 species with one strain and a genome of 600 to 780 bases each, and
two more species that the taxonomy holds but no genome (no DB k-mers). The oracle always works on
the pristine directory; the device works on copies, because mtb_em writes dbDir/sp2uniqKmerCnt.

Two references:
  * the oracle's emReassign (oc.em): sequential, the reference's own order;
  * em_reference below: Classifier::em + reclassify in doubles with every order of additions written
    out (np.add.accumulate is a strict left-to-right running sum). order="sequential" is the
    reference's order, held to tests/test_em.py's py_em and to the oracle bit for bit on the CPU.
    order="sliced" is the device's documented order: a species' contributions in query order, in
    consecutive slices of 4096, the slice sums added in order; and delta as k_em_delta adds it, 256
    chunks of ceil(S / 256) species, then the chunk sums in order. order="fsum" sums both exactly
    rounded (math.fsum) and is used for the record below only.

What is asserted. Where every species has at most 4096 mappings the device equals the oracle bit for
bit: abundances, query_count, iterations, emTaxCounts and every read's tax_id, mapped and score.
Where a species has more, the device equals em_reference(order="sliced") bit for bit. Every case
first asserts on the references alone that it reaches the path it is named for, and that no
iteration's delta lies within a factor 1 +- 1e-6 of the 1e-6 threshold (in the sequential, the sliced
and the exact sum), so that the iteration counts must agree whatever the order of delta's sum.

For the record (CPU, test_summation_orders_record; not a gate): largest relative difference of an
abundance over the slice cases with more than 4096 mappings in one species --
    sliced against the oracle's sequential order 4.0e-15, sliced against the exact sum 6.1e-16,
    sequential against the exact sum 3.8e-15,
and every such case's iteration counts are equal in all three. With 4097 mappings the two orders are
one (the second slice is a single addend); with 8192 and with 8193 they differ in the last bits. Each
slice case asserts its own half of that on the references (slice_case's check), so that neither of
the two larger cases can pass on a device that sums sequentially.

Out of scope, because the reference itself has no defined answer there: a species k-mer count of
exactly 1 (1 / log(1) is infinite and the reference then produces NaN); inputs in which no query has
a non-zero denominator (0 / 0 in the reference); species ids that the taxonomy does not hold.
"""
import ctypes
import functools
import math
import os
import shutil

import numpy as np
import pytest

from metabuli_work_amd import _abi, synth
from metabuli_work_amd._abi import default_params
from tests import oracle_ctypes as oc
from tests.test_em import _Tax, _count_file_text, _sp_kmers, py_em

K_SLICE = 4096   # mtb_em's kSlice
K_DELTA = 256    # k_em_delta's threads
N_SPECIES = 300


# ---------------------------------------------------------------------------------------------------
def _seq_sum(x):
    """x[0] + x[1] + ... from the left, as a C loop over doubles adds them."""
    return float(np.add.accumulate(np.asarray(x, np.float64))[-1]) if len(x) else 0.0


def em_reference(maps, sp_kmers, tax, total, order="sequential"):
    """Classifier::em + reclassify. Returns (reads, {top species: (abundance, emTaxCount)}, stats) as
    oc.em and Classifier.em do; stats also holds the per-iteration deltas and query counts."""
    assert order in ("sequential", "sliced", "fsum")
    maps = np.ascontiguousarray(maps, _abi.EM_MAP_DTYPE)
    n = len(maps)
    reads = np.zeros(total, _abi.EM_READ_DTYPE)
    if n == 0:  # no species: one iteration whose delta is an empty sum
        return reads, {}, {"query_count": 0, "iterations": 1, "deltas": [0.0], "query_counts": [0],
                           "absd0": np.zeros(0)}
    q, sp, sc = maps["query_id"], maps["species_id"], maps["score"].astype(np.float64)
    starts = np.flatnonzero(np.r_[True, q[1:] != q[:-1]])
    ends = np.r_[starts[1:], n]
    nQ = len(starts)
    qidx = np.repeat(np.arange(nQ), ends - starts)
    col = np.arange(n) - starts[qidx]
    width = int(col.max()) + 1
    cols = [np.flatnonzero(col == j) for j in range(width)]
    species = np.unique(sp)
    S = len(species)
    si = np.searchsorted(species, sp)
    top = np.zeros(S, bool)
    top[si[starts]] = True
    lf = np.array([1.0 / math.log(sp_kmers[int(s)]) if sp_kmers.get(int(s), 0) > 0 else 0.0 for s in species])
    p = np.where(top, 1.0 / int(top.sum()), 0.0)
    perm = np.argsort(si, kind="stable")  # species order, query order inside a species
    bounds = np.searchsorted(si[perm], np.arange(S + 1))

    def per_query(term):  # a query's terms added in mapping order
        den = np.zeros(nQ)
        for c in cols:
            den[qidx[c]] = den[qidx[c]] + term[c]
        return den

    def species_sum(x):
        if order == "fsum":
            return math.fsum(x)
        if order == "sliced":
            return _seq_sum([_seq_sum(x[a:a + K_SLICE]) for a in range(0, len(x), K_SLICE)])
        return _seq_sum(x)

    def delta_sum(absd):
        if order == "fsum":
            return math.fsum(absd)
        if order == "sliced":
            per = (S + K_DELTA - 1) // K_DELTA
            return _seq_sum([_seq_sum(absd[a:a + per]) for a in range(0, K_DELTA * per, per)])
        return _seq_sum(absd[top])

    deltas, qcs, absd0 = [], [], None
    qc = 0
    for it in range(1000):
        term = sc * p[si] * lf[si]
        den = per_query(term)
        counted = den != 0.0
        qc = int(counted.sum())
        w = np.where(counted[qidx], term / np.where(counted, den, 1.0)[qidx], 0.0)[perm]
        f = np.array([species_sum(w[bounds[i]:bounds[i + 1]]) for i in range(S)])
        f[top] = f[top] / float(qc)
        absd = np.where(top, np.abs(f - p), 0.0)
        delta = delta_sum(absd)
        if it == 0:
            absd0 = absd  # the first iteration's |f - p| per species, in species order
        if it > 10:
            f[top & (f < 1e-5)] = 0.0
        p = f
        deltas.append(delta)
        qcs.append(qc)
        if delta < 1e-6:
            break
    counts = (p * float(qc)).astype(np.int64)
    # reclassify
    term = p[si] * sc * lf[si]
    den = per_query(term)
    lca = functools.lru_cache(maxsize=None)(lambda cand: tax.lca(list(cand)))
    for k in range(nQ):
        a, b = starts[k], ends[k]
        if den[k] == 0.0:
            reads[q[a]] = (0, 2, 0.0)
            continue
        pr = term[a:b] / den[k]
        tot, cand = 0.0, []
        for j in sorted(range(b - a), key=lambda j: -pr[j]):  # <= 10 entries: libstdc++'s insertion sort, stable
            if tot >= 0.5:
                break
            tot += float(pr[j])
            cand.append(int(sp[a + j]))
        reads[q[a]] = (lca(tuple(cand)), 1, tot)
    out = {int(species[i]): (float(p[i]), int(counts[i])) for i in range(S) if top[i]}
    return reads, out, {"query_count": qc, "iterations": len(deltas), "deltas": deltas, "query_counts": qcs,
                       "absd0": absd0}


def assert_same(got, want, what):
    """Bit for bit: abundances, emTaxCounts, query_count, iterations, and per read tax_id, mapped, score."""
    (g_reads, g_sp, g_st), (w_reads, w_sp, w_st) = got, want
    assert g_st["iterations"] == w_st["iterations"], what
    assert g_st["query_count"] == w_st["query_count"], what
    assert list(g_sp) == list(w_sp), what
    ga, wa = np.array([v[0] for v in g_sp.values()]), np.array([v[0] for v in w_sp.values()])
    bad = np.flatnonzero(ga.view(np.uint64) != wa.view(np.uint64))
    assert len(bad) == 0, f"{what}: abundances differ at {[(list(w_sp)[i], ga[i], wa[i]) for i in bad[:5]]}"
    assert [v[1] for v in g_sp.values()] == [v[1] for v in w_sp.values()], what
    assert len(g_reads) == len(w_reads), what
    assert np.array_equal(g_reads["tax_id"], w_reads["tax_id"]), what
    assert np.array_equal(g_reads["mapped"], w_reads["mapped"]), what
    bad = np.flatnonzero(g_reads["score"].view(np.uint64) != w_reads["score"].view(np.uint64))
    assert len(bad) == 0, f"{what}: read scores differ at {bad[:5]}"


# ---------------------------------------------------------------------------------------------------
class Env:
    """The DB, its copies, the species and the Python-side counts."""

    def __init__(self, root):
        taxo = synth.make_taxonomy(N_SPECIES, 1, seed=41)
        gen = synth.make_genomes(taxo, genome_len=600, seed=42)
        genus = [t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "genus"]
        nxt = int(taxo.taxid.max()) + 1
        self.bare = [nxt, nxt + 1]  # species of the taxonomy without a genome: no DB k-mers
        taxo = synth.Taxonomy(np.concatenate([taxo.taxid, np.array(self.bare, np.int32)]),
                              np.concatenate([taxo.parent, np.array([genus[0], genus[5]], np.int32)]),
                              taxo.rank + ["species"] * 2, taxo.name + [f"species_{t}" for t in self.bare])
        self.base = os.path.join(root, "base")  # the oracle's: never gets the count file
        oc.build_db(self.base, default_params(kmer_format=2), taxo, gen)
        self.tax = _Tax(taxo)
        self.max_tax = int(taxo.taxid.max())
        self.counts = dict(_sp_kmers(self.base, self.tax))
        self.sp = sorted(t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "species" and t not in self.bare)
        assert len(self.sp) == N_SPECIES and all(self.counts.get(s, 0) > 1 for s in self.sp)
        assert not any(b in self.counts for b in self.bare)
        self.dev = os.path.join(root, "dev")  # the device's: mtb_em writes sp2uniqKmerCnt here
        shutil.copytree(self.base, self.dev)
        # a hand-written count file: chosen counts (four species alike), a 0, a taxID past maxTax
        self.hand = os.path.join(root, "hand")
        shutil.copytree(self.base, self.hand)
        self.zero = self.sp[7]
        # two pairs of sister species (a0, a1 in one genus, a2, a3 in another): the LCA tells which two led
        by_genus = {}
        for s in self.sp[:7] + self.sp[8:90] + self.sp[140:160]:
            by_genus.setdefault(self.tax.parent[s], []).append(s)
        pairs = [v[:2] for v in by_genus.values() if len(v) >= 2]
        assert len(pairs) >= 2
        self.alike = pairs[0] + pairs[1]
        self.most = max(self.sp[160:], key=lambda s: self.counts[s])  # apart from _background's species
        self.hand_counts = dict(self.counts)
        for s in self.alike:
            self.hand_counts[s] = 1000
        self.hand_counts[self.zero] = 0
        with open(os.path.join(self.hand, "sp2uniqKmerCnt"), "w") as f:
            for s in sorted(self.hand_counts):
                f.write(f"{s} {self.hand_counts[s]}\n")
            f.write(f"{self.max_tax + 7} 555\n")
        self.dirs = {"plain": (self.base, self.dev, self.counts), "hand": (self.hand, self.hand, self.hand_counts)}
        self._odb, self._ref = {}, {}

    def odb(self, db):
        if db not in self._odb:
            self._odb[db] = oc.OracleDb(self.dirs[db][0])
        return self._odb[db]

    def refs(self, name):
        """(case, oracle's result, em_reference sequential, em_reference sliced), computed once."""
        if name not in self._ref:
            c = CASES[name](self)
            db = c.get("db", "plain")
            maps, total = c["maps"], c["total"]
            self._ref[name] = (c, oc.em(self.odb(db), maps, total),
                               em_reference(maps, self.dirs[db][2], self.tax, total, "sequential"),
                               em_reference(maps, self.dirs[db][2], self.tax, total, "sliced"))
        return self._ref[name]

    def close(self):
        for o in self._odb.values():
            o.close()


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    e = Env(str(tmp_path_factory.mktemp("em_designed")))
    yield e
    e.close()


@pytest.fixture(scope="module")
def device(env):
    """One em context per DB directory, opened when first asked for."""
    from metabuli_work_amd.classifier import Classifier, LocalParameters
    ctx = {}

    def get(db):
        if db not in ctx:
            d = env.dirs[db][1]
            ctx[db] = Classifier(LocalParameters(seqMode=2, em=1).load_db_parameters(d), db_dir=d)
        return ctx[db]
    yield get
    for c in ctx.values():
        c.close()


def make_maps(rows):
    """rows: (query id, [(species, score), ...]) in query order."""
    out = np.zeros(sum(len(r) for _, r in rows), _abi.EM_MAP_DTYPE)
    k = 0
    for qid, r in rows:
        for s, v in r:
            out[k] = (qid, s, v)
            k += 1
    return out


def _scores(rng, n):
    return rng.uniform(0.05, 1.0, n).astype(np.float32)


def _background(e, rng, rows, n, first_id):
    """n two-species queries over species 100..139, so that a case's abundances are not trivial."""
    for i in range(n):
        a, b = e.sp[100 + i % 40], e.sp[100 + (i * 7 + 3) % 40]
        v = _scores(rng, 2)
        rows.append((first_id + i, [(a, float(v[0])), (b, float(v[1]))]))
    return first_id + n


# ---- the cases: name -> builder(env) -> {maps, total, db, check(case, oracle, seq, sliced)} ----------
def _per_species(maps):
    return np.unique(maps["species_id"], return_counts=True)


def slice_case(n_big):
    def build(e):
        rng = np.random.default_rng(n_big)
        big = e.sp[10]
        rows = []
        # the big species and twenty others share two reads of three; each also has reads of its own,
        # so the abundances settle inside (0, 1) and the shared reads' contributions stay fractions
        for i in range(n_big):
            other = e.sp[20 + i % 20]
            v = _scores(rng, 2)
            pair = [(big, float(v[0])), (other, float(v[1]))]
            rows.append((i, pair[:1] if i % 3 == 0 else pair if i % 7 == 0 else pair[::-1]))
        for j in range(200):
            rows.append((n_big + j, [(e.sp[20 + j % 20], float(_scores(rng, 1)[0]))]))
        total = _background(e, rng, rows, 60, n_big + 200)

        def check(c, orc, seq, sl):
            sp, cnt = _per_species(c["maps"])
            assert cnt.max() == n_big and sp[cnt.argmax()] == big and np.sort(cnt)[-2] <= 420
            assert (n_big + K_SLICE - 1) // K_SLICE == {4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3}[n_big]
            assert seq[2]["iterations"] > 3 and 0.05 < orc[1][big][0] < 0.99
            frac = orc[0]["score"][:n_big]  # a shared read's leading posterior: not 0, 0.5 or 1
            assert ((frac > 0.5) & (frac < 1.0)).sum() > n_big // 4
            # past one whole slice and a single addend the two orders must round differently, or the
            # case could not tell a device that sums sequentially from one that sums in slices
            a_seq = np.array([v[0] for v in seq[1].values()]).view(np.uint64)
            a_sl = np.array([v[0] for v in sl[1].values()]).view(np.uint64)
            assert list(seq[1]) == list(sl[1])
            if n_big > K_SLICE + 1:
                assert (a_seq != a_sl).any(), "sliced and sequential abundances are bit-identical"
            else:  # one slice, or one slice and a single addend: the same additions in the same order
                assert (a_seq == a_sl).all()
        return {"maps": make_maps(rows), "total": total, "check": check}
    return build


def species_case(S):
    def build(e):
        rng = np.random.default_rng(1000 + S)
        rows = []
        for i in range(2 * S + 5):
            a, b = e.sp[i % S], e.sp[(i * 3 + 1) % S]
            v = _scores(rng, 2)
            rows.append((i, [(a, float(v[0]))] if S == 1 else [(a, float(v[0])), (b, float(v[1]))]))

        def check(c, orc, seq, sl):
            sp, cnt = _per_species(c["maps"])
            assert len(sp) == S and len(orc[1]) == S and cnt.max() <= K_SLICE
            if S == 1:  # p = f = 1 from the start: delta is 0 after one iteration
                assert seq[2]["iterations"] == 1 and seq[2]["deltas"] == [0.0]
            else:
                assert seq[2]["iterations"] > 2
            per = (S + K_DELTA - 1) // K_DELTA
            absd0 = sl[2]["absd0"]
            assert len(absd0) == S and per == (2 if S > K_DELTA else 1)
            if S > K_DELTA:
                # k_em_delta's threads each add two species, and species past the first 256 take part in
                # the first iteration's delta: a kernel that stopped at 256 species would give another sum
                assert absd0[K_DELTA:].min() > 0.0
                assert (S + per - 1) // per < K_DELTA  # the last threads add nothing
        return {"maps": make_maps(rows), "total": 2 * S + 5, "check": check}
    return build


def zeroing_case(e):
    """Two species share 3000 queries with unequal scores (slow convergence). Z is the first mapping of
    three of them with a tiny score and the only mapping of one query: its abundance stays near
    1 / queries < 1e-5, so it is zeroed after iteration 10, and its own query's denominator with it."""
    rng = np.random.default_rng(77)
    A, B, Z = e.sp[50], e.sp[60], e.sp[70]
    n_fill = 120000
    q = np.arange(n_fill, dtype=np.uint32)
    fill = np.zeros(n_fill, _abi.EM_MAP_DTYPE)
    fill["query_id"], fill["species_id"] = q, np.array(e.sp, np.int32)[80 + q % 200]
    fill["score"] = _scores(rng, n_fill)
    rows = []
    for i in range(3000):
        r = [(A, 0.5), (B, 0.42)] if i % 2 else [(B, 0.42), (A, 0.5)]
        if i in (10, 20, 30):
            r = [(Z, 1e-6)] + r
        rows.append((n_fill + i, r))
    z_only = n_fill + 3000
    rows.append((z_only, [(Z, 0.9)]))
    maps = np.concatenate([fill, make_maps(rows)])
    nq = z_only + 1

    def check(c, orc, seq, sl):
        reads, sp, st = orc
        assert _per_species(c["maps"])[1].max() <= K_SLICE
        assert st["iterations"] > 12
        assert sp[Z][0] == 0.0 and sp[A][0] > 0.0
        assert reads["mapped"][z_only] == 2 and reads["tax_id"][z_only] == 0
        assert st["query_count"] == nq - 1 and seq[2]["query_counts"][0] == nq
    return {"maps": maps, "total": nq, "check": check}


def bare_top_case(db):
    def build(e):
        """A top species without DB k-mers (no genome; with the hand-written file: a 0 entry): its
        queries have a zero denominator from the first iteration on."""
        rng = np.random.default_rng(5)
        none = e.bare[0] if db == "plain" else e.zero
        A = e.sp[12]
        rows = [(0, [(none, 0.7)]), (1, [(none, 0.6), (A, 0.4)]), (2, [(A, 0.5), (none, 0.9)])]
        if db == "plain":
            rows.append((3, [(e.bare[1], 0.3), (e.bare[0], 0.3)]))
        nxt = _background(e, rng, rows, 50, 4)

        def check(c, orc, seq, sl):
            reads, sp, st = orc
            assert e.dirs[db][2].get(none, 0) == 0 and none in sp and sp[none] == (0.0, 0)
            assert seq[2]["query_counts"][0] == st["query_count"] < len(np.unique(c["maps"]["query_id"]))
            assert reads["mapped"][0] == 2 and reads["mapped"][1] == 1 and reads["tax_id"][1] == A
        return {"maps": make_maps(rows), "total": nxt, "db": db, "check": check}
    return build


def non_top_case(e):
    """Species that no query has first: abundance 0 throughout, absent from the returned list."""
    rng = np.random.default_rng(6)
    A, N1, N2 = e.sp[30], e.sp[31], e.sp[2]
    rows = [(i, [(A, 0.5), (N1, 0.8), (N2, 0.9)]) for i in range(5)]
    nxt = _background(e, rng, rows, 50, 5)

    def check(c, orc, seq, sl):
        reads, sp, st = orc
        assert {N1, N2} <= set(c["maps"]["species_id"].tolist()) and N1 not in sp and N2 not in sp
        assert (reads["tax_id"][:5] == A).all() and (reads["score"][:5] == 1.0).all()
    return {"maps": make_maps(rows), "total": nxt, "check": check}


def twice_case(e):
    """The same species twice within one query."""
    rng = np.random.default_rng(8)
    A, B = e.sp[33], e.sp[34]
    rows = [(0, [(A, 0.5), (A, 0.3), (B, 0.2)]), (1, [(B, 0.6), (A, 0.1), (B, 0.6)]), (2, [(A, 0.4), (A, 0.4)])]
    nxt = _background(e, rng, rows, 40, 3)

    def check(c, orc, seq, sl):
        assert orc[0]["mapped"][:3].tolist() == [1, 1, 1] and orc[0]["score"][2] == 0.5
    return {"maps": make_maps(rows), "total": nxt, "check": check}


def reclassify_case(e):
    """Equal posterior products at the 0.5 boundary (four species with the same k-mer count in
    symmetric queries: the sort's tie order picks the candidates and so the LCA), a query with one
    mapping, one with ten, query ids with gaps and reads past the last id."""
    rng = np.random.default_rng(9)
    a = e.alike
    rows, qid = [], 2
    perms = [(0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 0, 1), (3, 2, 1, 0), (0, 2, 1, 3), (1, 3, 0, 2), (2, 0, 3, 1), (3, 1, 2, 0)]
    four = []
    for rep in range(3):
        for pm in perms:
            rows.append((qid, [(a[i], 0.25) for i in pm]))
            four.append((qid, pm))
            qid += 3  # gaps
    two = []
    for pm in ((0, 1), (1, 0), (2, 3), (3, 2)):
        rows.append((qid, [(a[i], 0.75) for i in pm]))
        two.append((qid, pm))
        qid += 2
    single, ten = qid, qid + 5
    rows.append((single, [(e.sp[90], 0.3)]))
    rows.append((ten, [(e.sp[200 + 7 * j], float(0.9 - 0.07 * j)) for j in range(10)]))
    nxt = _background(e, rng, rows, 30, ten + 4)
    total = nxt + 9

    def check(c, orc, seq, sl):
        reads, sp, st = orc
        assert len({sp[s][0] for s in a}) == 1 and sp[a[0]][0] > 0  # the four abundances are one number
        used = np.unique(c["maps"]["query_id"])
        untouched = np.setdiff1d(np.arange(total), used)
        assert len(untouched) > 9 and untouched.max() == total - 1
        for f in ("tax_id", "mapped"):
            assert not reads[f][untouched].any()
        assert not reads["score"][untouched].any()
        got_two = {reads["tax_id"][qq] for qq, _ in two}
        assert all(reads["score"][qq] == 0.5 for qq, _ in two) and got_two == set(a)  # the first mapping wins
        for qq, pm in four:  # the candidates are a prefix of the mapping order (a stable sort of equal keys)
            k = int(round(reads["score"][qq] / 0.25))
            assert k in (2, 3) and reads["tax_id"][qq] == e.tax.lca([a[i] for i in pm[:k]])
        assert len({int(reads["tax_id"][qq]) for qq, _ in four}) > 1
        assert reads["mapped"][single] == 1 and reads["tax_id"][single] == e.sp[90] and reads["score"][single] == 1.0
        assert reads["mapped"][ten] == 1 and (c["maps"]["query_id"] == ten).sum() == 10
    return {"maps": make_maps(rows), "total": total, "db": "hand", "check": check}


def hand_file_case(e):
    """Every count from the hand-written file: the chosen counts, the 0 and the ignored taxID."""
    rng = np.random.default_rng(10)
    # A and X always together with equal scores: the one with fewer k-mers takes all of their reads.
    # From `info` that is A; the file gives A 1000 k-mers, more than X has.
    A, X = e.alike[0], e.most
    rows = [(i, [(A, 0.5), (X, 0.5)] if i % 2 else [(X, 0.5), (A, 0.5)]) for i in range(20)]
    rows.append((20, [(e.zero, 0.5), (e.sp[101], 0.2)]))
    nxt = _background(e, rng, rows, 60, 21)

    def check(c, orc, seq, sl):
        plain = em_reference(c["maps"], e.counts, e.tax, c["total"])
        assert e.counts[A] < e.counts[X] < e.hand_counts[A]
        assert plain[1][A][0] > 0.1 and plain[1][X][0] == 0.0, "from info, A takes the shared reads"
        assert seq[1][X][0] > 0.1 and seq[1][A][0] == 0.0, "with the file, X does"
        assert orc[1][e.zero] == (0.0, 0)
    return {"maps": make_maps(rows), "total": nxt, "db": "hand", "check": check}


def empty_case(total):
    def build(e):
        def check(c, orc, seq, sl):
            reads, sp, st = orc
            assert st == {"query_count": 0, "iterations": 1} and sp == {} and len(reads) == total
            assert not reads["tax_id"].any() and not reads["mapped"].any() and not reads["score"].any()
        return {"maps": np.zeros(0, _abi.EM_MAP_DTYPE), "total": total, "check": check}
    return build


def ten_case(e):
    """Exactly ten mappings per query (the most Reporter::writeMappings stores)."""
    rng = np.random.default_rng(11)
    rows = [(i, [(e.sp[(13 * i + 17 * j) % 250], float(v)) for j, v in enumerate(_scores(rng, 10))]) for i in range(40)]

    def check(c, orc, seq, sl):
        assert np.unique(c["maps"]["query_id"], return_counts=True)[1].tolist() == [10] * 40
    return {"maps": make_maps(rows), "total": 40, "check": check}


CASES = {f"slice_{n}": slice_case(n) for n in (4095, 4096, 4097, 8192, 8193)}
CASES.update({f"species_{s}": species_case(s) for s in (1, 255, 256, 257, 300)})
CASES.update({"zeroing": zeroing_case, "bare_top": bare_top_case("plain"), "zero_in_file": bare_top_case("hand"),
              "non_top": non_top_case, "twice": twice_case, "reclassify": reclassify_case, "hand_file": hand_file_case,
              "no_maps": empty_case(5), "no_reads": empty_case(0), "ten_per_query": ten_case})
SLICED = ("slice_4097", "slice_8192", "slice_8193")  # a species with more than 4096 mappings


def _strip(ref):
    return ref[0], ref[1], {k: ref[2][k] for k in ("query_count", "iterations")}


def _clear_of_threshold(deltas):
    return all(not (1e-6 * (1 - 1e-6) <= d <= 1e-6 * (1 + 1e-6)) for d in deltas)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_on_references(env, name):
    """CPU. The case reaches its path; the oracle equals the sequential restatement bit for bit (with
    the hand-written count file too: the oracle reads it as Classifier.cpp:393-411 does); no delta is
    at the threshold, in either order of its sum."""
    c, orc, seq, sl = env.refs(name)
    assert_same(orc, _strip(seq), name)
    c["check"](c, orc, seq, sl)
    exact = em_reference(c["maps"], env.dirs[c.get("db", "plain")][2], env.tax, c["total"], "fsum")
    for r in (seq, sl, exact):
        assert _clear_of_threshold(r[2]["deltas"]), (name, r[2]["deltas"][-3:])
    assert seq[2]["iterations"] == sl[2]["iterations"] == exact[2]["iterations"]
    if name not in SLICED:
        assert_same(_strip(sl), _strip(seq), name)  # up to 4096 mappings per species the two orders are one


def test_em_reference_against_py_em(env):
    """CPU. em_reference's sequential order is tests/test_em.py's py_em, bit for bit."""
    for name in ("species_255", "bare_top", "twice", "reclassify", "non_top"):
        c, orc, seq, sl = env.refs(name)
        counts = env.dirs[c.get("db", "plain")][2]
        reads, sp, st = py_em(c["maps"], counts, env.tax, c["total"])
        assert_same((reads, sp, st), _strip(seq), name)


def test_oracle_reads_count_file(env):
    """CPU. The oracle takes dbDir/sp2uniqKmerCnt when it is there: chosen counts, the 0 entry, the
    taxID past maxTax skipped; and counts from `info` when it is not."""
    c, orc, seq, sl = env.refs("hand_file")
    assert not os.path.exists(os.path.join(env.base, "sp2uniqKmerCnt"))
    assert_same(orc, _strip(seq), "file")
    plain = oc.em(env.odb("plain"), c["maps"], c["total"])
    assert_same(plain, _strip(em_reference(c["maps"], env.counts, env.tax, c["total"])), "info")
    assert plain[1] != orc[1]


def test_summation_orders_record(env):
    """CPU. How far the sliced order, the sequential order and the exact sum are from one another
    (printed; the figures are in this file's docstring and DESIGN.md)."""
    def rel(x, y):
        a, b = np.array([v[0] for v in x[1].values()]), np.array([v[0] for v in y[1].values()])
        return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
    worst = [0.0, 0.0, 0.0]
    for name in SLICED:
        c, orc, seq, sl = env.refs(name)
        exact = em_reference(c["maps"], env.counts, env.tax, c["total"], "fsum")
        d = (rel(sl, orc), rel(sl, exact), rel(seq, exact))
        print(f"{name}: sliced vs oracle {d[0]:.2e}, sliced vs fsum {d[1]:.2e}, sequential vs fsum {d[2]:.2e}, "
              f"iterations {sl[2]['iterations']} / {orc[2]['iterations']} / {exact[2]['iterations']}")
        worst = [max(w, x) for w, x in zip(worst, d)]
    print("worst: sliced vs oracle %.2e, sliced vs fsum %.2e, sequential vs fsum %.2e" % tuple(worst))
    assert all(math.isfinite(w) for w in worst)  # a record, not a gate: the sizes are not bounded here


# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_case_on_device(env, device, name):
    c, orc, seq, sl = env.refs(name)
    c["check"](c, orc, seq, sl)  # the case reaches its path, on the references alone
    got = device(c.get("db", "plain")).em(c["maps"], c["total"])
    got = got[0], got[1], {k: got[2][k] for k in ("query_count", "iterations")}
    if name in SLICED:
        assert_same(got, _strip(sl), name + " against the sliced order")
    else:
        assert_same(got, orc, name + " against the oracle")


@pytest.mark.gpu
def test_eleven_mappings_rejected(env, device):
    c = env.refs("ten_per_query")[0]
    m = c["maps"][:11].copy()
    m["query_id"] = 0
    from metabuli_work_amd._lib import MtbError
    with pytest.raises(MtbError, match="more than 10 mappings for one query"):
        device("plain").em(m, 40)
    device("plain").em(m[:10], 40)


@pytest.mark.gpu
def test_species_capacity_retry(env, device):
    """A species capacity below the number of top species: MTB_RETRY with n_sp set (through the C-ABI:
    Classifier.em always sizes enough)."""
    from metabuli_work_amd._lib import lib
    c, orc, seq, sl = env.refs("species_255")
    maps, total = np.ascontiguousarray(c["maps"]), c["total"]
    reads = np.zeros(total, _abi.EM_READ_DTYPE)
    for cap in (0, 254):
        ids, probs, cnts = np.zeros(255, np.int32), np.zeros(255, np.float64), np.zeros(255, np.uint32)
        nsp, st = ctypes.c_uint64(0), _abi.MtbEmStats()
        rc = lib().mtb_em(device("plain").handle, maps.ctypes.data, len(maps), total, reads.ctypes.data, ids.ctypes.data,
                          probs.ctypes.data, cnts.ctypes.data, cap, ctypes.byref(nsp), ctypes.byref(st))
        assert rc == _abi.MTB_RETRY and nsp.value == 255 and st.n_species == 255
        assert not ids.any() and not probs.any()
    rc = lib().mtb_em(device("plain").handle, maps.ctypes.data, len(maps), total, reads.ctypes.data, ids.ctypes.data,
                      probs.ctypes.data, cnts.ctypes.data, 255, ctypes.byref(nsp), ctypes.byref(st))
    assert rc == _abi.MTB_OK and ids.tolist() == list(orc[1])


@pytest.mark.gpu
def test_species_kmers_file(env, tmp_path):
    """On a fresh copy of the DB without the file, one em writes sp2uniqKmerCnt: line for line the
    counts computed in Python from `info` and the taxonomy (k_species_kmers against a reference of its
    own)."""
    from metabuli_work_amd.classifier import Classifier, LocalParameters
    d = str(tmp_path / "fresh")
    shutil.copytree(env.base, d)
    path = os.path.join(d, "sp2uniqKmerCnt")
    assert not os.path.exists(path)
    c, orc, seq, sl = env.refs("twice")
    with Classifier(LocalParameters(seqMode=2, em=1).load_db_parameters(d), db_dir=d) as clf:
        got = clf.em(c["maps"], c["total"])
    assert_same((got[0], got[1], {k: got[2][k] for k in ("query_count", "iterations")}), orc, "fresh copy")
    assert open(path).read() == _count_file_text(env.base, env.tax) and len(env.counts) == N_SPECIES


@pytest.mark.gpu
@pytest.mark.parametrize("db_name", ["fmt2", "fmt2_acc", "fmt1_acc", "fmt2_syncmer", "fmt1"])
def test_species_kmers_file_shared_dbs(make_db, tmp_path, db_name):
    """The same on fresh copies of the suite's shared DBs, where k_species_kmers has more to do: two
    strains per species, accession-level leaves under the strains (several taxa of `info` into one
    species), k-mer format 1 and syncmers. The file the device writes equals, line for line, the
    counts made in Python from `info` and the taxonomy, and its EM over a few designed mappings
    equals, bit for bit, the oracle's on a second copy that never holds the file (the oracle counts
    from `info` itself there) and the Python restatement's with those counts."""
    from metabuli_work_amd.classifier import Classifier, LocalParameters
    db_dir, taxo, gen = make_db(db_name)
    dev_dir, orc_dir = str(tmp_path / "dev"), str(tmp_path / "orc")
    for d in (dev_dir, orc_dir):
        shutil.copytree(db_dir, d, ignore=shutil.ignore_patterns("sp2uniqKmerCnt"))
    tax = _Tax(taxo)
    counts = dict(_sp_kmers(orc_dir, tax))
    species = sorted(counts)
    # reached: every species gathers k-mers of more than one taxon of `info`, and counts differ
    taxa_of = {}
    for t in np.unique(np.fromfile(os.path.join(orc_dir, "info"), np.uint32)).tolist():
        taxa_of.setdefault(tax.species(int(t)), set()).add(int(t))
    assert len(species) >= 10 and all(len(taxa_of[s]) >= 2 for s in species) and len(set(counts.values())) > 1
    assert all(k > 1 for k in counts.values())
    rng = np.random.default_rng(len(db_name))
    rows = []
    for i in range(6 * len(species)):
        a, b = species[i % len(species)], species[(5 * i + 2) % len(species)]
        v = _scores(rng, 2)
        rows.append((i, [(a, float(v[0])), (b, float(v[1]))]))
    maps, total = make_maps(rows), len(rows) + 2
    odb = oc.OracleDb(orc_dir)
    orc = oc.em(odb, maps, total)
    odb.close()
    assert_same(orc, _strip(em_reference(maps, counts, tax, total)), db_name + ": oracle against Python")
    assert orc[2]["iterations"] > 2 and len(orc[1]) == len(species)
    par = LocalParameters(seqMode=2, em=1).load_db_parameters(dev_dir)
    with Classifier(par, db_dir=dev_dir) as clf:
        got = clf.em(maps, total)
    assert open(os.path.join(dev_dir, "sp2uniqKmerCnt")).read() == _count_file_text(orc_dir, tax)
    assert not os.path.exists(os.path.join(orc_dir, "sp2uniqKmerCnt"))
    assert_same((got[0], got[1], {k: got[2][k] for k in ("query_count", "iterations")}), orc, db_name)
