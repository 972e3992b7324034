"""Paired batches whose mates differ in length, against the oracle at every stage.

The other parity tests sample their pairs with both mates of one nominal length; the only short mates
are 5-25 bases cut from a 150-bp pair and the only long inputs are single-end. The hot path assumes
more than those batches exercise:

* a pair with a mate below one window (25 bases or fewer) is dropped by the shared empty rule and adds
  nothing to the batch's largest window count, whatever its other mate's length: the batch keeps
  uniform units (12 units per pair, K4 rebuilds a matched query's info from its slot and the mate
  lengths) and K1F stages each block's bases in LDS (kSeqStage = 10240 bytes, mtb_launch.h);
* in a uniform batch a matched query's info comes from the two mate lengths, 16 bits each;
* in a non-uniform paired batch a read's units split as 6 * c1 then 6 * c2 chunks.

Every batch here is made by hand from sampled pairs and genome substrings, holds at most 64 reads,
and is compared with the oracle as test_stage_parity compares: query k-mers with their info, matches
in compareMatches order, results and taxID:count lists, the non-blank query k-mer count; then the
same batch once more on the same context. One context takes all the paired batches of a DB format in
turn (units are chosen per batch: uniform after non-uniform and the reverse must leave no state).
"""
import ctypes

import numpy as np
import pytest

from metabuli_work_amd import _abi, synth
from metabuli_work_amd._abi import KMER_DTYPE, MATCH_DTYPE, TAXCNT_DTYPE, info_seq, ptr
from tests import oracle_ctypes as oc

N_BASE = 44      # pairs of a mixed batch: 528 units, K1F blocks 0..2 (256 units each)
ODD = (0, 21, 43)  # first pair, the pair whose 12 units (252..263) straddle blocks 0 and 1, last pair
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def covered(length):
    """getMaxCoveredLength (LocalUtil.h:45-52): the bases of a mate the six frames cover."""
    return length - {2: 2, 1: 4, 0: 3}[length % 3]


def _revcomp(s):
    return COMP[s[::-1]]


def _sub(gen, g, start, length):
    """`length` bases of genome g from `start`."""
    a, b = int(gen.off[g]), int(gen.off[g + 1])
    assert a + start + length <= b
    return np.asarray(gen.seq[a + start:a + start + length], np.uint8)


def _genome_pair(gen, k, len1, len2):
    """A pair cut from the first genome from k % n on that is long enough: mate 1 forward, mate 2 the
    reverse complement of a stretch that starts where mate 1 starts (both lie in the genome whatever
    their lengths)."""
    glens = np.diff(gen.off).astype(np.int64)
    g = next(j % gen.n for j in range(k, k + gen.n) if glens[j % gen.n] >= max(len1, len2))
    glen = int(glens[g])
    start = (977 * k) % max(1, glen - max(len1, len2) + 1)
    return _sub(gen, g, start, len1), _revcomp(_sub(gen, g, start, len2))


def _reads(m1, m2=None):
    def pack(ms):
        off = np.zeros(len(ms) + 1, np.uint64)
        off[1:] = np.cumsum([len(m) for m in ms])
        return np.concatenate(ms).astype(np.uint8), off
    s1, o1 = pack(m1)
    s2, o2 = pack(m2) if m2 is not None else (None, None)
    return synth.Reads(s1, o1, s2, o2, np.full(len(m1), -1, np.int32))


class Case:
    def __init__(self, name, reads, mode=2, empty=None, classified=(), mixed=False, uniform=None, nothing=False,
                 matched=()):
        self.name, self.reads, self.mode = name, reads, mode
        self.matched = matched        # reads that must have matches (cut from the genomes)
        self.empty = empty or {}      # read index -> query_length of a pair the empty rule drops
        self.classified = classified  # reads that must classify
        self.mixed = mixed            # a batch of N_BASE pairs, most of which must classify
        self.uniform = uniform        # uniform_units the batch takes when the layout is on (None: not asserted)
        self.nothing = nothing        # no query k-mer at all


def build_cases(gen):
    """The batches, in the order one context takes them (uniform and non-uniform ones alternate)."""
    base = synth.make_reads(gen, 60, seed=5)  # 150/150 pairs
    b1 = [np.asarray(base.seq1[int(base.off1[i]):int(base.off1[i + 1])]) for i in range(N_BASE)]
    b2 = [np.asarray(base.seq2[int(base.off2[i]):int(base.off2[i + 1])]) for i in range(N_BASE)]
    assert all(len(a) == 150 and len(b) == 150 for a, b in zip(b1, b2))
    long_all = np.asarray(gen.seq, np.uint8)

    def mixed(name, odd, **kw):
        """The 44 sampled pairs with pair i replaced by odd[i] = (mate 1, mate 2)."""
        m1, m2 = list(b1), list(b2)
        for i, (a, b) in odd.items():
            m1[i], m2[i] = a, b
        return Case(name, _reads(m1, m2), mixed=True, **kw)

    def empty_pair(len1, len2, k=0):
        """A pair with a mate below one window: its long mate from the genomes, its short one too."""
        a, b = _genome_pair(gen, k, min(len1, 20000), min(len2, 20000))
        if len1 > 20000:
            a = long_all[:len1]
        if len2 > 20000:
            b = long_all[:len2]
        return a, b

    def ql(len1, len2):
        return covered(len1) + covered(len2)

    cases = []
    # a long mate beside a mate without a window, in the first pair, in the pair across the first block
    # boundary and in the last: the batch stays uniform
    for name, l1, l2 in (("long_m1_empty_m2", 5000, 15), ("empty_m1_long_m2", 25, 5000)):
        cases.append(mixed(name, {i: empty_pair(l1, l2, i) for i in ODD}, empty={i: ql(l1, l2) for i in ODD},
                           uniform=12))
    # unequal chunk counts (non-uniform): c1 = 312 chunks beside c2 = 1, and the reverse
    nonuni = {0: _genome_pair(gen, 3, 20000, 26), 43: _genome_pair(gen, 8, 20000, 26),
              21: _genome_pair(gen, 5, 26, 20000), 5: _genome_pair(gen, 6, 218, 30),
              30: _genome_pair(gen, 7, 3000, 500)}
    cases.append(mixed("unequal_nonuniform", nonuni, classified=(0, 43), uniform=0))
    # block 0 holds the units of pairs 0..21: 21 pairs of 150/150 (6300 bases) and an empty pair that
    # brings the block's bases to exactly kSeqStage = 10240, and to one more. With the stage taken only by
    # batches whose mates are all at most kSeqMate = 219 bases (launch_extract_filter's seqFits, from
    # k_read_meta's second word), the bound that decides the kernel is the longest mate: 219 bases stage in
    # LDS (23 pairs * 2 * 219 = 10074 <= 10240), 220 read HBM; one batch on each side of that too
    for name, l1 in (("stage_bound_10240", 3930), ("stage_bound_10241", 3931), ("mate_bound_219", 219),
                     ("mate_bound_220", 220)):
        cases.append(mixed(name, {21: empty_pair(l1, 10, 2)}, empty={21: ql(l1, 10)}, uniform=12))
    # nothing but empty pairs with long mates: maxW = 0, chunk C = 1
    pairs = [empty_pair(5000, 4, k) for k in range(4)]
    cases.append(Case("all_empty_long", _reads([a for a, _ in pairs], [b for _, b in pairs]),
                      empty={i: ql(5000, 4) for i in range(4)}, uniform=12, nothing=True))
    # a mate past the 16-bit length field of readLens, in an empty pair: its neighbours are unaffected
    cases.append(mixed("len_clamp", {21: empty_pair(70000, 10)}, empty={21: ql(70000, 10)}, uniform=12))
    # mates at the window threshold: 25 bases hold no window, 26 hold one per frame
    thr = [(26, 25), (25, 26), (26, 26)]
    pairs = [_genome_pair(gen, k, *thr[k % 3]) for k in range(36)]
    cases.append(Case("threshold_mates", _reads([a for a, _ in pairs], [b for _, b in pairs]),
                      empty={k: ql(*thr[k % 3]) for k in range(36) if k % 3 != 2}, uniform=12))
    # a uniform batch, every pair with mates of two lengths, all from the genomes: a matched query's info is
    # rebuilt from the slot and both lengths
    lens = [(217, 26), (26, 217), (100, 151), (151, 100), (60, 213), (215, 216)]
    pairs = [_genome_pair(gen, k, *lens[k % 6]) for k in range(48)]
    cases.append(Case("unequal_uniform", _reads([a for a, _ in pairs], [b for _, b in pairs]), uniform=12,
                      matched=tuple(range(48))))
    # the non-uniform batch once more, after uniform ones
    cases.append(mixed("unequal_nonuniform_again", nonuni, classified=(0, 43), uniform=0))
    # single-end, 6 units per read: read 42's units (252..257) straddle blocks 0 and 1, and it is the one
    # without a window
    sl = [26 + (i * 191) // 63 for i in range(64)]
    sl[42] = 25
    assert min(sl) == 25 and max(sl) == 217
    cases.append(Case("single_straddle", _reads([_genome_pair(gen, k, L, 1)[0] for k, L in enumerate(sl)]), mode=1,
                      empty={42: covered(25)}, uniform=6))
    return cases


def check_oracle_alone(case, ores, omatches):
    """What keeps the GPU comparison from being "both sides empty"."""
    cls = ores["is_classified"] != 0
    with_matches = set(info_seq(omatches["qinfo"]).tolist())
    for i in case.matched:
        assert i + 1 in with_matches, f"{case.name}: read {i} has no match"
    for i, q in case.empty.items():
        assert not cls[i], f"{case.name}: empty pair {i} classified"
        assert int(ores["query_length"][i]) == q, f"{case.name}: read {i} query_length"
    for i in case.classified:
        assert cls[i], f"{case.name}: read {i} is not classified"
    if case.mixed:
        assert int(cls.sum()) >= 30, f"{case.name}: {int(cls.sum())} of {N_BASE} classified"
    if case.nothing:
        assert not cls.any()


def test_query_length_examples():
    """The covered lengths the issue quotes for the empty pairs."""
    assert covered(5000) + covered(15) == 5010
    assert covered(70000) + covered(10) == 70002
    assert covered(20000) + covered(26) == 20022


def test_oracle_on_odd_batches(make_db):
    """The oracle alone on the fmt2 batches: most pairs of a mixed batch classify, every empty pair
    stays unclassified with query_length = covered(len1) + covered(len2), the 20000/26 pairs classify."""
    from tests.test_gpu_parity import _params
    db_dir, taxo, gen = make_db("fmt2")
    odb = oc.OracleDb(db_dir)
    seen = set()
    for case in build_cases(gen):
        par = _params(db_dir, case.mode)
        okmers, omatches, ores, otc = _oracle_stages(odb, par, case.reads)
        check_oracle_alone(case, ores, omatches)
        cres, ctc = oc.classify(odb, par.to_c(), case.reads)  # the one-call path agrees with the staged one
        assert np.array_equal(cres, ores) and np.array_equal(ctc, otc)
        seen.add(case.name)
        if case.name == "long_m1_empty_m2":
            assert [int(ores["query_length"][i]) for i in ODD] == [5010] * 3
        if case.name == "len_clamp":
            assert int(ores["query_length"][21]) == 70002
        if case.name == "unequal_nonuniform":
            assert int(ores["query_length"][0]) == 20022 and ores["is_classified"][0]
    odb.close()
    assert {"long_m1_empty_m2", "empty_m1_long_m2", "stage_bound_10240", "stage_bound_10241", "all_empty_long",
            "len_clamp", "threshold_mates", "unequal_uniform", "unequal_nonuniform", "single_straddle"} <= seen


def test_stage_bound_batches_sit_on_the_bound(make_db):
    """Block 0 of the stage_bound batches (the units of pairs 0..21) holds 10240 and 10241 bases."""
    db_dir, taxo, gen = make_db("fmt2")
    by = {c.name: c for c in build_cases(gen)}
    for name, want in (("stage_bound_10240", 10240), ("stage_bound_10241", 10241)):
        r = by[name].reads
        last = (256 - 1) // 12  # the read of block 0's last unit
        assert last == 21 and int(r.off1[last + 1]) + int(r.off2[last + 1]) == want


KNOBS = {
    "default": {},
    "no_uniform": {"MTB_UNIFORM_UNITS": "0"},
    "seq_hbm": {"MTB_K1F_SEQ_LDS": "0"},
    "unstaged_join": {"MTB_MATCH_WINDOW": "0"},
    "binned": {"MTB_K1F_BINS": "2"},
}


def _compare(clf, case, br, par, db_dir, o, knobs):
    """One classified batch (keep_stages) against the oracle's stages; returns the failures."""
    from tests.test_gpu_parity import _kmer_sorted, compare_results, okmers_present
    okmers, omatches, ores, otc = o
    bad = []

    def step(what, fn):
        try:
            fn()
        except AssertionError as e:
            bad.append(f"{what}: {str(e)[:300]}")

    def kmers():
        gk = clf.query_kmers()
        ok = okmers_present(okmers, db_dir, par)
        assert len(gk) == len(ok) == clf.stats()["query_kmers"], f"{len(gk)} query k-mers, oracle {len(ok)}"
        assert np.array_equal(_kmer_sorted(gk), _kmer_sorted(ok)), "query k-mers (value, info) differ"
        assert br.query_kmers == int((info_seq(okmers["info"]) != 0).sum()), "non-blank query k-mer count"
        if case.nothing:
            assert len(gk) == 0 and br.query_kmers == 0

    def matches():
        gm = clf.matches()
        assert len(gm) == len(omatches) == br.matches, f"{len(gm)} matches, oracle {len(omatches)}"
        assert np.array_equal(gm, omatches), "matches differ (compareMatches order)"

    def results():
        compare_results(br.results, br.taxcnt, ores, otc)
        if case.nothing:
            assert not br.results["is_classified"].any()
        for i in case.classified:
            assert br.results["is_classified"][i], f"read {i} not classified"

    def units():
        if case.uniform is not None:
            want = 0 if knobs.get("MTB_UNIFORM_UNITS") == "0" else case.uniform
            assert clf.stats()["uniform_units"] == want, f"uniform_units {clf.stats()['uniform_units']} != {want}"

    step("k-mers", kmers)
    step("matches", matches)
    step("results", results)
    step("units", units)
    return bad


def _oracle_stages(odb, par, reads):
    opar = par.to_c()
    okmers, ql1, ql2 = oc.extract(opar, reads)
    omatches = oc.match(odb, opar, okmers)
    ores, otc = oc.assign(odb, opar, omatches, ql1, ql2)
    return okmers, omatches, ores, otc


@pytest.fixture(scope="module")
def oracle_cases(make_db):
    """Per DB format: (db_dir, [(case, params, oracle stages)]), computed once for every knob set."""
    from tests.test_gpu_parity import _params
    cache = {}

    def get(db_name):
        if db_name not in cache:
            db_dir, taxo, gen = make_db(db_name)
            odb = oc.OracleDb(db_dir)
            out = []
            for case in build_cases(gen):
                par = _params(db_dir, case.mode)
                out.append((case, par, _oracle_stages(odb, par, case.reads)))
            odb.close()
            cache[db_name] = (db_dir, out)
        return cache[db_name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("db_name", ["fmt2", "fmt1"])
def test_odd_batches_stage_parity(oracle_cases, monkeypatch, db_name, knobs):
    """Every batch of build_cases through one context per read mode, each twice, against the oracle's
    k-mers, matches and results; under the default knobs, without uniform units, with K1F's bases read
    from HBM, with the unstaged join, and with K1F writing K2's buckets."""
    from metabuli_work_amd.classifier import Classifier
    from metabuli_work_amd._lib import MtbError
    for k, v in KNOBS[knobs].items():
        monkeypatch.setenv(k, v)
    db_dir, cases = oracle_cases(db_name)
    failures = []
    for mode in (2, 1):
        todo = [c for c in cases if c[0].mode == mode]
        with Classifier(todo[0][1], db_dir=db_dir) as clf:
            for case, par, o in todo:
                check_oracle_alone(case, o[2], o[1])
                r = case.reads
                for run in (1, 2):
                    try:
                        br = clf.classify_batch(r.seq1, r.off1, r.seq2, r.off2, keep_stages=True)
                    except MtbError as e:
                        failures.append(f"{case.name} run {run}: {e}")
                        continue
                    failures += [f"{case.name} run {run}: {b}" for b in _compare(clf, case, br, par, db_dir, o,
                                                                                 KNOBS[knobs])]
    assert not failures, "\n".join(failures)


# ---- the C-ABI getters at exact capacity ------------------------------------------------------------
PATTERN = 0xA5
GUARD = 64


def _guarded(n, itemsize):
    return np.full(n * itemsize + GUARD, PATTERN, np.uint8)


def _exact_capacity(L, h, name, fn, dtype, n, want):
    """fn(handle, out, capacity, n_out): exact capacity, one short, and (n == 0) no buffer at all."""
    bad = []
    nout = ctypes.c_uint64(~0 & 0xFFFFFFFFFFFFFFFF)
    buf = _guarded(n, dtype.itemsize)
    rc = fn(h, ptr(buf), n, ctypes.byref(nout))
    if rc != _abi.MTB_OK or nout.value != n:
        bad.append(f"{name}: capacity n = {n}: rc {rc}, n_out {nout.value}")
    if not (buf[n * dtype.itemsize:] == PATTERN).all():
        bad.append(f"{name}: wrote past {n} records")
    if rc == _abi.MTB_OK and want is not None and not np.array_equal(buf[:n * dtype.itemsize].view(dtype), want):
        bad.append(f"{name}: records differ from the wrapper's")
    if n > 0:
        buf = _guarded(n - 1, dtype.itemsize)
        nout = ctypes.c_uint64(0)
        rc = fn(h, ptr(buf), n - 1, ctypes.byref(nout))
        if rc != _abi.MTB_RETRY or nout.value != n:
            bad.append(f"{name}: capacity n - 1: rc {rc} (MTB_RETRY {_abi.MTB_RETRY}), n_out {nout.value} != {n}")
        if not (buf == PATTERN).all():
            bad.append(f"{name}: capacity n - 1: buffer written")
    else:
        nout = ctypes.c_uint64(7)
        rc = fn(h, ctypes.c_void_p(0), 0, ctypes.byref(nout))
        if rc != _abi.MTB_OK or nout.value != 0:
            bad.append(f"{name}: n == 0, NULL out: rc {rc}, n_out {nout.value}")
    return bad


def _short_by_one(name, fn, ctype, offers):
    """fn(out, n) with n one less than the getter offers: element n stays the pattern."""
    size = ctypes.sizeof(ctype)
    buf = np.full(offers * size, PATTERN, np.uint8)
    fn(buf.ctypes.data_as(ctypes.POINTER(ctype)), offers - 1)
    return [] if (buf[(offers - 1) * size:] == PATTERN).all() else [f"{name}: wrote past element n - 1"]


@pytest.mark.gpu
def test_getters_exact_capacity(oracle_cases):
    """mtb_get_taxcnt / mtb_get_query_kmers / mtb_get_matches / mtb_copy_taxcnt through raw ctypes after a
    uniform batch, a non-uniform one and one without a query k-mer: a buffer of exactly n records is
    filled and nothing behind it; one record short gives MTB_RETRY with *n_out = n and an untouched
    buffer; n = 0 needs no buffer. The fixed-size getters write no more than the n they are given."""
    from metabuli_work_amd.classifier import Classifier
    from metabuli_work_amd._lib import lib
    L = lib()
    db_dir, cases = oracle_cases("fmt2")
    by = {c[0].name: c for c in cases}
    bad = []
    with Classifier(by["unequal_uniform"][1], db_dir=db_dir) as clf:
        h = clf.handle
        for name in ("unequal_uniform", "unequal_nonuniform", "all_empty_long"):
            case, par, o = by[name]
            r = case.reads
            clf.classify_batch(r.seq1, r.off1, r.seq2, r.off2, keep_stages=True)
            st = clf.stats()
            assert st["uniform_units"] == case.uniform
            nq, nm, nt = st["query_kmers"], clf.last_counts()[1], clf.n_taxcnt()
            if case.nothing:
                assert (nq, nm, nt) == (0, 0, 0)
            else:
                assert nq > 0 and nm > 0 and nt > 0
            got = [_exact_capacity(L, h, "mtb_get_taxcnt", L.mtb_get_taxcnt, TAXCNT_DTYPE, nt, clf.taxcnt()),
                   _exact_capacity(L, h, "mtb_get_query_kmers", L.mtb_get_query_kmers, KMER_DTYPE, nq,
                                   clf.query_kmers()),
                   _exact_capacity(L, h, "mtb_get_matches", L.mtb_get_matches, MATCH_DTYPE, nm, clf.matches())]
            # mtb_copy_taxcnt takes no capacity: exactly n records, and no buffer when there are none
            buf = _guarded(nt, TAXCNT_DTYPE.itemsize)
            nout = ctypes.c_uint64(7)
            rc = L.mtb_copy_taxcnt(h, ptr(buf), 0, ctypes.byref(nout))
            if rc != _abi.MTB_OK or nout.value != nt or not (buf[nt * TAXCNT_DTYPE.itemsize:] == PATTERN).all():
                got.append([f"mtb_copy_taxcnt: rc {rc}, n_out {nout.value} != {nt}, or wrote past its records"])
            elif not np.array_equal(buf[:nt * TAXCNT_DTYPE.itemsize].view(TAXCNT_DTYPE), clf.taxcnt()):
                got.append(["mtb_copy_taxcnt: records differ from mtb_get_taxcnt's"])
            if nt == 0:
                nout = ctypes.c_uint64(7)
                rc = L.mtb_copy_taxcnt(h, ctypes.c_void_p(0), 0, ctypes.byref(nout))
                if rc != _abi.MTB_OK or nout.value != 0:
                    got.append([f"mtb_copy_taxcnt: n == 0, NULL dst: rc {rc}, n_out {nout.value}"])
            got += [_short_by_one("mtb_last_stats", lambda p, n: L.mtb_last_stats(h, p, n), ctypes.c_uint64,
                                  len(clf.STATS)),
                    _short_by_one("mtb_last_stage_ms", lambda p, n: L.mtb_last_stage_ms(h, p, n), ctypes.c_float, 5),
                    _short_by_one("mtb_last_kernel_ms", lambda p, n: L.mtb_last_kernel_ms(h, p, n), ctypes.c_float, 7),
                    _short_by_one("mtb_open_phases", lambda p, n: L.mtb_open_phases(h, p, n), ctypes.c_double,
                                  len(clf.OPEN_PHASES)),
                    _short_by_one("mtb_merge_last_ms", lambda p, n: L.mtb_merge_last_ms(p, n), ctypes.c_float, 5)]
            bad += [f"{name}: {b}" for g in got for b in g]
    assert not bad, "\n".join(bad)
