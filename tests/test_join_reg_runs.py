"""k_join_uniform's register path (MTB_JOIN_REG_RUN = R: a DB run of up to R records is selected and
emitted from registers, a run of R + 1 .. 48 by the lane's loop, a longer one by k_match_long) at its
edges, on designed DBs of a few thousand k-mers.

The DBs are made of families as tests/golden/ref_match.npz's are (one AA 8-mer as N synonymous 24-nt
variants, each a one-window gene block under a strain of another species), here over the amino acids
with four codons only (A, G, P, T, V): two synonymous codons of those always differ in the third base, a
Hamming distance of 1 (hammingLookup rows 0-3), so a query's Hamming sum against a record is the number
of codons in which they differ and a selection can be designed. A family of n <= 6 is a centre C (not in
the DB) and members C with codon i changed, i < n. Its queries:
  C itself                       every sum 1, threshold 2: every candidate selected
  member j                       sum 0, threshold 0: that record alone, at each position of the run
  C with codons 0 and 1 changed  members 0 and 1 tied at 1, the others at 3 > 2
  C with every codon changed     every sum 8, threshold 7: no candidate
  member 0 with 1, 2, 3 changes  one record at Hamming 1; every record (threshold 4, 6)
Families of 1 .. 6 records (R - 1 .. R + 2 for R = 3 and 4) and of 47, 48 and 49 (kLongRun is 48); the
family of the smallest AA 8-mer (4 records) is the DB's first records, that of the largest (4 records in
DB "last4", 5 in "last5") its last: the last DB k-mer is never a candidate, so those runs hold 3 and 4
candidates. Each read holds one member window between random flanks, on either strand: one kept query.

Batches: the first 1, 63, 64, 65 and 129 reads of the shuffled pool, the whole pool, 33-bp reads (whose
quartered stretches the register path's matches spill past under MTB_DIRECT=3), and for each R a
batch of 192 queries over five families whose AA 8-mers differ in their first letter (so their order
in the sorted batch is theirs whatever the sort's low bits do): 64 queries of a run of R (a wave of
n = R alone), 1 of a run of R + 1 (lane 0 of the next wave), 63 + 63 of runs of R, 1 of a run of R + 1
(lane 63 of the third wave). The CPU test counts all of this from the oracle and the decoded DB."""
import functools
import os
import tempfile

import numpy as np
import pytest

from metabuli_work_amd import synth
from metabuli_work_amd._abi import default_params
from tests import oracle_ctypes as oc
from tests import pyscan
from tests import ref_match_fixture as fx
from tests.build_cases import _case

CODONS = {"A": ["GCT", "GCC", "GCA", "GCG"], "G": ["GGT", "GGC", "GGA", "GGG"], "P": ["CCT", "CCC", "CCA", "CCG"],
          "T": ["ACT", "ACC", "ACA", "ACG"], "V": ["GTT", "GTC", "GTA", "GTG"]}
COMP = str.maketrans("ACGT", "TGCA")
# hammingLookup (KmerMatcher.h:66-70)
LUT = np.array([[0, 1, 1, 1, 2, 1, 3, 3], [1, 0, 1, 1, 2, 2, 3, 2], [1, 1, 0, 1, 2, 2, 2, 3], [1, 1, 1, 0, 1, 2, 3, 3],
                [2, 2, 2, 1, 0, 1, 4, 4], [1, 2, 2, 2, 1, 0, 4, 4], [3, 3, 2, 3, 4, 4, 0, 1], [3, 2, 3, 3, 4, 4, 1, 0]])
LONG_RUN = 48  # kLongRun
REG_RUNS = (2, 3, 4)
CLASSES = (1, 2, 3, 4, 5, 6, 47, 48, 49)
SHAPES = (1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def _tmp():  # made when a DB is first built, not at collection
    return tempfile.TemporaryDirectory(prefix="mtb_reg_runs_")


def _dna(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _value(s24):
    (v, _), = pyscan.block_windows(s24.encode(), 0, 23, True, 2, 0, 5)
    return v


class Family:
    def __init__(self, rng, aas, n):
        self.aas, self.n = aas, n
        self.centre = [int(x) for x in rng.integers(0, 4, 8)]
        if n <= 8:
            self.members = [self.changed(self.centre, [i]) for i in range(n)]
        else:  # distinct random variants
            seen = set()
            while len(seen) < n:
                seen.add(tuple(int(x) for x in rng.integers(0, 4, 8)))
            self.members = [list(c) for c in sorted(seen)]

    @staticmethod
    def changed(c, at, by=1):
        c = list(c)
        for i in at:
            c[i] = (c[i] + by) % 4
        return c

    def dna(self, c):
        return "".join(CODONS[a][i] for a, i in zip(self.aas, c))

    def queries(self):
        """(24-nt window, what it is there for)."""
        m0 = self.members[0]
        q = [(m, "member") for m in self.members[:6]] + [(self.changed(m0, [7], 2), "1 change")]
        if self.n <= 8:
            q += [(self.centre, "centre"), (self.changed(self.centre, range(8), 2), "far"),
                  (self.changed(m0, [6, 7], 2), "2 changes"), (self.changed(m0, [5, 6, 7], 2), "3 changes")]
            if self.n >= 2:
                q.append((self.changed(self.centre, [0, 1]), "tied"))
        return [(self.dna(c), why) for c, why in q]


@functools.lru_cache(maxsize=None)
def design(last):
    """The DB "last4" / "last5" (written once), its families and the read pools."""
    rng = np.random.default_rng(20261021)
    letters = sorted(CODONS, key=lambda a: _value(CODONS[a][0] * 8))  # by AA index
    used = set()

    def fam(aas, n):
        assert aas not in used
        used.add(aas)
        return Family(rng, aas, n)

    def rand_aas():
        while True:
            aas = "".join(letters[i] for i in rng.integers(0, 5, 8))
            if aas not in used and aas[:2] not in (letters[0] * 2, letters[-1] * 2):
                return aas
    # the smallest and the largest AA 8-mer of the DB: no other begins with the first or last letter twice (not
    # that letter eight times: the other strand of GCN GCN ... reads GCN again one base on, and the tails are
    # random for the same reason)
    def tail(n):
        return "".join(letters[i] for i in rng.integers(0, 5, n))
    first, lastf = fam(letters[0] * 2 + tail(6), 4), fam(letters[-1] * 2 + tail(6), 5 if last == "last5" else 4)
    # the wave batches: five families per R in the order of their first letters, runs of R, R + 1, R, R, R + 1
    waves = {R: [fam(letters[i] + letters[k + 1] + tail(6), n) for i, n in enumerate((R, R + 1, R, R, R + 1))]
             for k, R in enumerate(REG_RUNS)}
    general = [fam(rand_aas(), n) for n in (1, 2, 3, 4, 5, 6) for _ in range(4)] + [fam(rand_aas(), n) for n in (47, 48, 49)]
    filler = [fam(rand_aas(), 1) for _ in range(2500)]
    taxo = synth.make_taxonomy(12, 2, seed=21)
    strains = [t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "no rank" and t != 1]
    seqs, taxids, blocks = [], [], []
    for f in [first, lastf] + [w for R in REG_RUNS for w in waves[R]] + general + filler:
        for i, c in enumerate(f.members):  # each member under a strain of another species (2 strains per species)
            seqs.append(np.frombuffer((_dna(rng, 6) + f.dna(c) + _dna(rng, 6)).encode(), np.uint8))
            taxids.append(strains[(2 * i + len(seqs) % 2) % len(strains)])
            blocks.append((len(seqs) - 1, 6, 29, 1))
    case = _case("reg_runs_" + last, taxo, seqs, taxids, blocks)
    d = os.path.join(_tmp().name, last)
    oc.build_db(d, default_params(kmer_format=2), case.taxo, case.gen, split_num=64)

    def read(window, k, flank=15):  # ATG beside the window: no shifted window of the frame is in the DB
        s = _dna(rng, flank) + "ATG" + window + "ATG" + _dna(rng, 15 if flank else 3)
        return s[::-1].translate(COMP) if k % 2 else s
    pool = [(f, w, why) for f in [first, lastf] + general for w, why in f.queries()]
    pool = [pool[i] for i in rng.permutation(len(pool))]
    pool_reads = [read(w, k) for k, (_, w, _) in enumerate(pool)]
    wave_reads = {}
    for R in REG_RUNS:
        ws = []
        for f, cnt in zip(waves[R], (64, 1, 63, 63, 1)):
            q = f.queries()
            ws += [q[k % len(q)][0] for k in range(cnt)]
        order = rng.permutation(len(ws))
        wave_reads[R] = [read(ws[i], k) for k, i in enumerate(order)]
    # 33-bp reads (3 windows a frame: a read's stretch is 6 * 3 slots, a quarter of it under MTB_DIRECT=3), so
    # that queries emitted from registers spill
    # (single-end: past 4 matches; paired, both mates holding a window: past 9, so the runs of 5 and 6 whose every
    # record is selected come first, next to each other)
    short = [q for f in general if f.n in (5, 6) for q in f.queries() if q[1] == "centre"]
    short += [q for f in general if f.n <= 6 for q in f.queries() if q[1] in ("centre", "tied", "member")][::2]
    short_reads = [read(w, k, flank=0) for k, (w, _) in enumerate(short)]
    return d, pool_reads, wave_reads, [_dna(rng, 60) for _ in range(len(pool_reads) + 192)], short_reads


def batches(last):
    """name -> list of reads (each holds one window of the DB)."""
    _, pool, wave, _, short = design(last)
    out = {f"first{n}": pool[:n] for n in SHAPES}
    out["pool"] = pool
    out["short"] = short
    for R in REG_RUNS:
        out[f"wave{R}"] = wave[R]
    return out


def as_reads(last, name, paired):
    """synth.Reads of a batch; paired: the window's read is mate 1 or mate 2 in turn, the other mate random."""
    rs = batches(last)[name]
    other = design(last)[3]

    def pack(strs):
        off = np.zeros(len(strs) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in strs])
        return np.frombuffer("".join(strs).encode(), np.uint8).copy(), off
    if not paired:
        a, oa = pack(rs)
        return synth.Reads(a, oa, None, None, np.full(len(rs), -1, np.int32))
    if name == "short":  # both mates hold a window
        a, oa = pack(rs)
        b, ob = pack(rs[1:] + rs[:1])
        return synth.Reads(a, oa, b, ob, np.full(len(rs), -1, np.int32))
    a, oa = pack([r if k % 2 == 0 else other[k] for k, r in enumerate(rs)])
    b, ob = pack([other[k] if k % 2 == 0 else r for k, r in enumerate(rs)])
    return synth.Reads(a, oa, b, ob, np.full(len(rs), -1, np.int32))


def _params(d, paired):
    from metabuli_work_amd.classifier import LocalParameters
    return LocalParameters(seqMode=2 if paired else 1).load_db_parameters(d)


def ham_sums(q, values):
    s = np.zeros(len(values), np.int64)
    for i in range(8):
        s += LUT[(int(q) >> (3 * i)) & 7, ((values >> np.uint64(3 * i)) & np.uint64(7)).astype(np.int64)]
    return s


@functools.lru_cache(maxsize=None)
def expect(last, name, paired):
    """From the oracle's query list and the decoded DB: per kept query (in sorted order) its number of
    candidates and selection; and the oracle's matches, results and taxID:count lists."""
    d = design(last)[0]
    reads = as_reads(last, name, paired)
    par = _params(d, paired)
    values = fx.decode(np.fromfile(os.path.join(d, "diffIdx"), np.uint16))
    _, start, length, run_aa = fx.runs_of(values)
    length = length.copy()
    length[-1] -= 1  # the last DB k-mer is never a candidate
    kmers, _, _ = oc.extract(par.to_c(), reads)
    kmers = kmers[fx.info_seq(kmers["info"]) != 0]
    q_aa = kmers["value"] >> np.uint64(24)
    r = np.minimum(np.searchsorted(run_aa, q_aa), len(run_aa) - 1)
    kept = run_aa[r] == q_aa
    n = length[r[kept]]
    sel = []
    for qv, ri in zip(kmers["value"][kept].tolist(), r[kept].tolist()):
        s = ham_sums(qv, values[start[ri]:start[ri] + length[ri]])
        sel.append(tuple(int(x) for x in np.nonzero(s <= min(2 * s.min(), 7))[0]) if len(s) else ())
    odb = oc.OracleDb(d)
    om = oc.match(odb, par.to_c(), kmers)
    ores, otc = oc.classify(odb, par.to_c(), reads)
    odb.close()
    return dict(n=n, sel=sel, n_query=len(kmers), matches=om, results=ores, taxcnt=otc, D=len(values), run=r[kept],
                run_records=np.diff(np.append(start, len(values))))


def loop_waves(n, R):
    """64-query waves of the sorted kept queries that hold a lane with R < n <= kLongRun."""
    loop = (n > R) & (n <= LONG_RUN)
    return int(sum(loop[i:i + 64].any() for i in range(0, len(n), 64)))


def pattern(n, sel):
    if len(sel) == n:
        return "all" if n else "absent"
    return {0: "none", 1: f"one@{sel[0] if sel else 0}", 2: "two"}.get(len(sel), "some")


def test_inputs_cover_the_shapes():
    """Not an empty test: every run-length class has kept queries, every selection pattern occurs, the
    batches have their sizes and the wave batches their waves (in any order the sort leaves equal-prefix
    keys: each family's queries are one stretch, the families ordered by their first letter)."""
    seen = {}
    for last in ("last4", "last5"):
        for paired in (True, False):
            e = expect(last, "pool", paired)
            assert sum(len(s) for s in e["sel"]) == len(e["matches"])  # the model here selects what the oracle does
            for n, s in zip(e["n"].tolist(), e["sel"]):
                seen[(n, pattern(n, s))] = seen.get((n, pattern(n, s)), 0) + 1
        e = expect(last, "pool", True)
        assert 2000 <= e["D"] <= 5000
        # the clamped families: the DB's first run holds 4 records and its queries 4 candidates; its last run
        # holds 4 ("last4") or 5 ("last5") records and its queries one candidate fewer (3: registers under R >= 3;
        # 4: the loop under R = 3, registers under R = 4)
        n_last = 5 if last == "last5" else 4
        first_q, last_q = e["n"][e["run"] == 0], e["n"][e["run"] == len(e["run_records"]) - 1]
        assert e["run_records"][0] == 4 and len(first_q) >= 8 and (first_q == 4).all()
        assert e["run_records"][-1] == n_last and len(last_q) >= 8 and (last_q == n_last - 1).all()
        for k in SHAPES:
            for paired in (True, False):
                assert len(expect(last, f"first{k}", paired)["n"]) == k
        for R in REG_RUNS:
            n = expect(last, f"wave{R}", True)["n"]
            assert len(n) == 192 and (n[:64] == R).all()
            assert n[64] == R + 1 and (n[65:128] == R).all()
            assert (n[128:191] == R).all() and n[191] == R + 1
            assert loop_waves(n, R) == 2 and loop_waves(n, R + 1) == 0
            if R > 2:
                assert loop_waves(n, R - 1) == 3
    print()
    for k in sorted(seen):
        print(f"run of {k[0]:2d} candidates, {k[1]:6s}: {seen[k]} queries")
    for n in CLASSES:
        assert any(k[0] == n for k in seen), f"no kept query of a run of {n}"
    for n in (1, 2, 3, 4, 5, 6):
        need = ["all", "none"] + [f"one@{j}" for j in range(n)] + (["two"] if n >= 3 else [])
        if n == 1:
            need.remove("one@0")  # a run of one: selected ("all") or not
        for p in need:
            assert seen.get((n, p), 0) >= 1, f"run of {n}: no query selecting {p}"
    for n in (47, 48, 49):
        assert any(k[0] == n and k[1].startswith("one@") for k in seen)


FORMS = ["default", "spill", "ext"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
@pytest.mark.parametrize("last", ["last4", "last5"])
def test_join_reg_runs(last, paired, form, monkeypatch):
    from metabuli_work_amd.classifier import Classifier
    from tests.test_gpu_parity import compare_results
    from tests.test_ref_match import _set_form

    _set_form(monkeypatch, form)
    d = design(last)[0]
    par = _params(d, paired)
    with Classifier(par, db_dir=d) as clf:
        for name in batches(last):
            e = expect(last, name, paired)
            reads = as_reads(last, name, paired)
            for R in ("nofast",) + REG_RUNS:
                monkeypatch.setenv("MTB_JOIN_FAST", "0" if R == "nofast" else "1")
                monkeypatch.setenv("MTB_JOIN_REG_RUN", "4" if R == "nofast" else str(R))
                br = clf.classify_batch(reads.seq1, reads.off1, reads.seq2, reads.off2, keep_stages=True)
                gm, st = clf.matches(), clf.stats()
                what = f"{last} {name} paired={paired} {form} R={R}"
                assert st["uniform_units"] == (12 if paired else 6), what
                assert st["query_kmers"] == len(e["n"]) and br.query_kmers == e["n_query"], what
                assert len(gm) == len(e["matches"]) == br.matches, what
                assert np.array_equal(gm, e["matches"]), what
                compare_results(br.results, br.taxcnt, e["results"], e["taxcnt"])
                assert st["long_run_queries"] == int((e["n"] > LONG_RUN).sum()), what
                if R != "nofast":
                    loop = (e["n"] > R) & (e["n"] <= LONG_RUN)
                    assert st["loop_queries"] == int(loop.sum()), what
                    assert (st["loop_waves"] > 0) == bool(loop.any()) and st["loop_waves"] <= st["loop_queries"], what
                    if name.startswith("wave"):  # the families' order in the sorted batch is fixed: exact
                        assert st["loop_waves"] == loop_waves(e["n"], R), what
                if form == "spill" and name == "short":
                    assert st["spilled_matches"] > 0, what
