"""The merge against the reference's OWN mergeTargetFiles<DB_CREATION> (tests/golden/ref_merge.npz, written by
tests/golden/make_ref_merge.py from code cut out of the reference at run time; every committed case's
diffIdx / info / split came out byte-identical from six runs: one outer pass and many, 1, 3 and 16 threads).

CPU part: the numpy restatement the merge tests take their expected values from (tests/merge_expect.py)
reproduces the reference's three files byte for byte, so what tests/test_gpu_merge.py checks the device
against is the reference's rule and not its author's reading of it.
GPU part: mtb_merge_db / mtb_merge_db_dirs on the same cases; the chunked load of each input
(MTB_DECODE_CHUNK_WORDS) at chunk sizes that cut k-mers at every position; 64 inputs.

The fixture's `artefact` case is one whose many-pass runs differ from its one-pass runs because of the
reference's buffering (DESIGN, merge section); it is held to numpy with the one-pass bytes and kept out
of the device comparison. What the reference cannot answer (an empty input, a merge of one k-mer) stays
held to numpy."""
import functools
import os
import pathlib

import numpy as np
import pytest

from metabuli_work_amd import synth
from tests.dbref import Tree, decode_diff, diff_words
from tests.group_filter_cases import encode_diffidx
from tests.merge_expect import expected_merge, merge_rule_split

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "ref_merge.npz"
MTB_ERR_ARG, MTB_ERR_DB = -1, -4


@functools.lru_cache(maxsize=None)
def fixture():
    fx = np.load(GOLDEN)
    taxo = synth.make_taxonomy(int(fx["taxonomy"][0]), int(fx["taxonomy"][1]), seed=int(fx["taxonomy"][2]))
    # the taxonomy the reference ran on is the one the tests build
    assert np.array_equal(taxo.taxid, fx["tax_id"]) and np.array_equal(taxo.parent, fx["tax_parent"])
    assert list(taxo.rank) == fx["tax_rank"].tolist()
    return fx, taxo, Tree(taxo)


def case_names(comparable_only=False):
    fx = np.load(GOLDEN)
    return [c for c in fx["cases"].tolist() if not comparable_only or int(fx[f"{c}_comparable"])]


def case_inputs(fx, name):
    """[(diffIdx words, info)] of a case's inputs, in file order."""
    return [(fx[f"{name}_in{i}_diffIdx"], fx[f"{name}_in{i}_info"]) for i in range(int(fx[f"{name}_n_in"]))]


def restated(tree, inputs, split_num):
    """(diffIdx, info, split) by the numpy restatement."""
    parts = [(decode_diff(d), i) for d, i in inputs]
    ev, ei = expected_merge(tree, parts)
    return encode_diffidx(ev), ei, merge_rule_split(ev, sum(len(i) for _, i in inputs), split_num)


# ---- CPU: the restatement against the reference ---------------------------------------------------------
def test_fixture_holds_the_cases():
    """The cases the fixture must hold, and what each was built to show."""
    fx, _, tree = fixture()
    names = case_names()
    for n in (3, 5, 8):
        for kind in ("equal", "unequal"):
            c = f"in{n}_{kind}"
            assert c in names and int(fx[f"{c}_n_in"]) == n
            sizes = [len(i) for _, i in case_inputs(fx, c)]
            assert (len(set(sizes)) == 1) == (kind == "equal"), sizes
            # one (value, species) group with a member in every input
            keys = [set(zip(decode_diff(d).tolist(), tree.sp[i.astype(np.int64)].tolist())) for d, i in case_inputs(fx, c)]
            assert set.intersection(*keys), c
    for s in (4, 16, 64):
        for kind, total in (("total_sm2", s - 2), ("total_sm1", s - 1), ("total_2sm1", 2 * (s - 1))):
            c = f"s{s}_{kind}"
            assert int(fx[f"{c}_split_num"]) == s and sum(len(i) for _, i in case_inputs(fx, c)) == total
        assert not fx[f"s{s}_total_sm2_split"].any()  # sizeOfSplit 0: nothing written
        sp = fx[f"s{s}_dups_short_split"].reshape(-1, 3)
        total = sum(len(i) for _, i in case_inputs(fx, f"s{s}_dups_short"))
        assert len(fx[f"s{s}_dups_short_info"]) < (s - 1) * (total // (s - 1))  # the last offset is never reached
        assert (sp[1:, 1] != 0).sum() < s - 2
        # an offset inside the last AA run: the last k-mers share their AA part and one offset falls among them
        v = decode_diff(fx[f"s{s}_last_run_diffIdx"])
        run = int((v >> np.uint64(24) == v[-1] >> np.uint64(24)).sum())
        size = sum(len(i) for _, i in case_inputs(fx, f"s{s}_last_run")) // (s - 1)
        assert run > size and (len(v) - run) // size < (len(v) - 1) // size
        # AA runs straddling several offsets
        v = decode_diff(fx[f"s{s}_straddle_diffIdx"])
        size = sum(len(i) for _, i in case_inputs(fx, f"s{s}_straddle")) // (s - 1)
        _, runs = np.unique(v >> np.uint64(24), return_counts=True)
        assert runs.max() >= 2 * size
    # the last k-mer: a duplicate pair and a singleton
    for c, dup in (("last_dup", True), ("last_single", False)):
        parts = [(decode_diff(d), i) for d, i in case_inputs(fx, c)]
        top = max(int(v[-1]) for v, _ in parts)
        assert sum(int(v[-1]) == top for v, _ in parts) == (2 if dup else 1)
        assert int(decode_diff(fx[f"{c}_diffIdx"])[-1]) == top
        assert sum(len(i) for _, i in parts) // 16 > 100  # splitWidth at 16 threads
    assert len(fx["tiny_equal_info"]) == 1 and len(fx["tiny_unequal_info"]) == 2
    # the meetings of the two-input case
    (va, ia), (vb, ib) = [(decode_diff(d), i.astype(np.int64)) for d, i in case_inputs(fx, "two_meetings")]
    a = {}
    for v, t in zip(va.tolist(), ia.tolist()):
        a.setdefault(v, []).append(t)
    kinds = {"strains": 0, "same": 0, "species": 0}
    groups = {}
    for v, t in zip(vb.tolist(), ib.tolist()):
        for u in a.get(v, []):
            if u == t:
                kinds["same"] += 1
            elif tree.sp[u] == tree.sp[t]:
                kinds["strains"] += 1
            else:
                kinds["species"] += 1
    for v, t in list(zip(va.tolist(), ia.tolist())) + list(zip(vb.tolist(), ib.tolist())):
        groups.setdefault((v, int(tree.sp[t])), set()).add(t)
    assert all(k > 10 for k in kinds.values()), kinds
    assert any(len(g) >= 3 for g in groups.values())
    # a five-word delta is among the inputs' words and the outputs'
    assert any((diff_words(decode_diff(fx[f"{c}_diffIdx"])) == 5).any() for c in names)


@pytest.mark.parametrize("name", case_names())
def test_restatement_reproduces_the_reference(name):
    """expected_merge + merge_rule_split + the plain diffIdx encoder == the reference's diffIdx, info and
    split, byte for byte (for the artefact case: the reference's one-pass bytes)."""
    fx, _, tree = fixture()
    diff, info, split = restated(tree, case_inputs(fx, name), int(fx[f"{name}_split_num"]))
    assert diff.astype(np.uint16).tobytes() == fx[f"{name}_diffIdx"].tobytes()
    assert info.astype(np.uint32).tobytes() == fx[f"{name}_info"].tobytes()
    assert split.astype(np.uint64).tobytes() == fx[f"{name}_split"].tobytes()


def test_artefact_case_is_the_buffering_one():
    """The case kept out of the device comparison differs between the reference's settings only as DESIGN says:
    the many-pass runs wrote some (value, species) group in two pieces, so they hold the one-pass entries
    plus repeats of values that occur twice inside one input."""
    fx, _, tree = fixture()
    if "artefact" not in case_names():
        return
    one_v, many_v = decode_diff(fx["artefact_diffIdx"]), decode_diff(fx["artefact_many_diffIdx"])
    assert len(many_v) > len(one_v)
    key = lambda v, i: set(zip(v.tolist(), tree.sp[i.astype(np.int64)].tolist()))  # noqa: E731
    assert key(one_v, fx["artefact_info"]) == key(many_v, fx["artefact_many_info"])
    pairs, counts = np.unique(np.stack([many_v, tree.sp[fx["artefact_many_info"].astype(np.int64)].astype(np.uint64)], 1),
                              axis=0, return_counts=True)
    inside = set()
    for d, _ in case_inputs(fx, "artefact"):
        v, c = np.unique(decode_diff(d), return_counts=True)
        inside |= set(v[c >= 2].tolist())
    assert (counts > 1).any() and all(int(v) in inside for v in pairs[counts > 1, 0])


# ---- GPU ------------------------------------------------------------------------------------------------
def _host_dbs(fx, taxo, name):
    from metabuli_work_amd.dbbuild import HostDb
    dbs = []
    for d, i in case_inputs(fx, name):
        dbs.append(HostDb(taxo, d.copy(), i.copy(), np.zeros(3, np.uint64), np.unique(i).astype(np.int32)))
    return dbs


def _par():
    from metabuli_work_amd._abi import default_params
    return default_params(kmer_format=2)


def _merge(dbs, taxo, split_num, par=None):
    from metabuli_work_amd.dbbuild import merge_dbs
    return merge_dbs(dbs, taxo, par or _par(), device=0, split_num=split_num)


def _assert_is(m, diff, info, split, what):
    assert m.diff_idx.tobytes() == np.asarray(diff, np.uint16).tobytes(), what
    assert m.info.tobytes() == np.asarray(info, np.uint32).tobytes(), what
    assert np.asarray(m.split, np.uint64).tobytes() == np.asarray(split, np.uint64).tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", case_names(comparable_only=True))
def test_device_merge_equals_the_reference(name):
    """merge_dbs, inputs in file order and rotated by one: the reference's three files; the taxID list is the
    sorted union. kmer_format 1 and 2 run the same reference code (AminoAcidPart reads the format only for 3
    and 4), so both are held to the one result."""
    from metabuli_work_amd._abi import default_params
    fx, taxo, _ = fixture()
    dbs = _host_dbs(fx, taxo, name)
    split_num = int(fx[f"{name}_split_num"])
    union = np.unique(np.concatenate([d.taxid_list for d in dbs]))
    for order, fmt in ((dbs, 2), (dbs[1:] + dbs[:1], 2), (dbs, 1)):
        m = _merge(order, taxo, split_num, default_params(kmer_format=fmt))
        _assert_is(m, fx[f"{name}_diffIdx"], fx[f"{name}_info"], fx[f"{name}_split"], (name, fmt))
        assert np.array_equal(m.taxid_list, union) and np.all(np.diff(m.taxid_list) > 0)


@pytest.mark.gpu
def test_device_merge_db_dirs_equals_the_reference(tmp_path):
    from metabuli_work_amd.dbbuild import merge_db_dirs
    fx, taxo, _ = fixture()
    name = "in5_unequal"
    dirs = []
    for k, db in enumerate(_host_dbs(fx, taxo, name)):
        dirs.append(str(tmp_path / f"part{k}"))
        db.write(dirs[-1], _par())
    out = str(tmp_path / "merged")
    merge_db_dirs(dirs, out, device=0, split_num=int(fx[f"{name}_split_num"]))
    for f, dt in (("diffIdx", np.uint16), ("info", np.uint32), ("split", np.uint64)):
        assert np.fromfile(os.path.join(out, f), dt).tobytes() == fx[f"{name}_{f}"].tobytes(), f
    ids = np.loadtxt(os.path.join(out, "taxID_list"), dtype=np.int32, ndmin=1)
    assert np.array_equal(ids, np.unique(np.concatenate([i for _, i in case_inputs(fx, name)])))


# ---- the chunked load -----------------------------------------------------------------------------------
CHUNKS = ("8", "9", "999")


def _db(taxo, tree, values, taxids):
    """A HostDb from entries in compareTargetKmer order, by the plain encoder."""
    from metabuli_work_amd.dbbuild import HostDb
    v, t = np.asarray(values, np.uint64), np.asarray(taxids, np.int64)
    if len(v):
        assert np.array_equal(np.lexsort((t, tree.sp[t], v)), np.arange(len(v)))
    return HostDb(taxo, encode_diffidx(v), t.astype(np.uint32), np.zeros(3, np.uint64), np.unique(t).astype(np.int32))


def _expect(tree, dbs, split_num):
    return restated(tree, [(d.diff_idx, d.info) for d in dbs], split_num)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunked_load_fixture_cases(chunk, monkeypatch):
    """Every comparable fixture case with each input decoded in chunks of 8, 9 and 999 words: the reference's
    bytes, as unchunked."""
    fx, taxo, _ = fixture()
    monkeypatch.setenv("MTB_DECODE_CHUNK_WORDS", chunk)
    for name in case_names(comparable_only=True):
        m = _merge(_host_dbs(fx, taxo, name), taxo, int(fx[f"{name}_split_num"]))
        _assert_is(m, fx[f"{name}_diffIdx"], fx[f"{name}_info"], fx[f"{name}_split"], (name, chunk))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunked_load_tile_edges(chunk, monkeypatch):
    """test_gpu_merge's tile-edge inputs under the chunked load, against the same numpy expectation."""
    from metabuli_work_amd._lib import lib
    from tests.test_gpu_merge import SPLIT_NUM, pin_db, tile_cases
    taxo = synth.make_taxonomy(12, 3, seed=5)
    tree = Tree(taxo)
    T = int(lib().mtb_merge_tile_items())
    leaves = np.array([t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "no rank" and t != 1], np.int64)
    cases = {k: [pin_db(taxo, tree, *a), pin_db(taxo, tree, *b)] for k, (a, b) in tile_cases(T, leaves, tree).items()}
    expect = {k: _expect(tree, dbs, SPLIT_NUM) if sum(len(d.info) for d in dbs) else None for k, dbs in cases.items()}
    monkeypatch.setenv("MTB_DECODE_CHUNK_WORDS", chunk)
    for k, dbs in cases.items():
        m = _merge(dbs, taxo, SPLIT_NUM)
        if expect[k] is None:
            assert len(m.diff_idx) == 0 and len(m.info) == 0, k
        else:
            _assert_is(m, *expect[k], (k, chunk))


def _values_of_words(words, start=1):
    """Ascending values whose deltas take the given numbers of diffIdx words."""
    v, out = start, []
    for k, w in enumerate(words):
        v += (1 << 15 * (w - 1)) + k % 3
        out.append(v)
    assert out[-1] < 1 << 64
    out = np.array(out, np.uint64)
    assert diff_words(out).tolist()[1:] == list(words)[1:]
    return out


def _pattern_values(n, start=1):
    """n ascending values whose deltas take 1, 2, 3, 4, 5, 1, 2, ... words."""
    return _values_of_words(([1, 2, 3, 4, 5] * n)[:n], start)


# the pattern 1, 2, 3, 4, 5 restarted at these phases, period after period (found by trying: chunks of 8 and of 9
# words re-align with a strictly periodic pattern after one period and then cut at the same places for ever)
PHASES = (2, 4, 3, 0, 4, 3, 1, 4)


def _cut_offsets(words, W):
    """The chunked walk over k-mers of the given word counts: chunks of W words, each starting where the last
    whole k-mer of the one before ended. The offsets into five-word k-mers at which chunks end."""
    ends = np.cumsum(words)
    w0, cuts = 0, set()
    while w0 < ends[-1]:
        stop = min(w0 + W, int(ends[-1]))
        last = int(ends[ends <= stop][-1])
        k = int(np.searchsorted(ends, stop, side="left"))
        if last != stop and words[k] == 5:
            cuts.add(stop - last)
        w0 = last
    return cuts


@pytest.mark.gpu
def test_chunked_load_cuts_every_position(monkeypatch):
    """K-mers of 1, 2, 3, 4, 5 words in a repeating pattern, each period starting at one of PHASES: over the
    eight periods (120 words) chunks of 8 and of 9 words each end at every position inside a five-word k-mer
    (checked from the word counts). The second input is three words long: it shares the chunk temporaries
    sized by the larger."""
    _, taxo, tree = fixture()
    leaves = np.array([t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "no rank" and t != 1], np.int64)
    rng = np.random.default_rng(3)
    pattern = [1, 2, 3, 4, 5]
    words = np.array([w for p in PHASES for w in pattern[p:] + pattern[:p]])
    for W in (8, 9):
        assert _cut_offsets(words, W) == {1, 2, 3, 4}, (W, _cut_offsets(words, W))
    v = _values_of_words(words.tolist(), start=1 << 20)  # the first delta too takes its two words
    big = _db(taxo, tree, v, rng.choice(leaves, len(v)))
    small = _db(taxo, tree, _pattern_values(2, start=77), rng.choice(leaves, 2))
    assert big.diff_idx.size == 120 and diff_words(v).tolist() == words.tolist() and len(small.diff_idx) == 3
    exp = _expect(tree, [big, small], 4)
    for chunk in (None, "8", "9"):
        if chunk is None:
            monkeypatch.delenv("MTB_DECODE_CHUNK_WORDS", raising=False)
        else:
            monkeypatch.setenv("MTB_DECODE_CHUNK_WORDS", chunk)
        _assert_is(_merge([big, small], taxo, 4), *exp, chunk)
        _assert_is(_merge([small, big], taxo, 4), *exp, chunk)


@pytest.mark.gpu
def test_chunked_load_chunk_ending_on_a_terminator(monkeypatch):
    """Eight one-word k-mers, then more: with W = 8 the first (a middle) chunk's last word is itself a
    terminator (lastTerm == n - 1 before the end), and the next chunk starts on a fresh k-mer."""
    _, taxo, tree = fixture()
    leaves = np.array([t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "no rank" and t != 1], np.int64)
    rng = np.random.default_rng(4)
    v = np.concatenate([np.arange(1, 17, dtype=np.uint64), np.uint64(16) + _pattern_values(10)])
    a = _db(taxo, tree, v, rng.choice(leaves, len(v)))
    assert (a.diff_idx[:16] >> 15).all() and len(a.diff_idx) > 24
    b = _db(taxo, tree, v[::3] + np.uint64(2), rng.choice(leaves, len(v[::3])))
    exp = _expect(tree, [a, b], 4)
    for chunk in ("8", "16", "9"):
        monkeypatch.setenv("MTB_DECODE_CHUNK_WORDS", chunk)
        _assert_is(_merge([a, b], taxo, 4), *exp, chunk)


def _refused(dbs, taxo, code, *says):
    from metabuli_work_amd._lib import MtbError, lib
    with pytest.raises(MtbError) as e:
        _merge(dbs, taxo, 16)
    msg = lib().mtb_last_error().decode()
    assert f"({code})" in str(e.value), str(e.value)
    assert msg != ""
    for s in says:
        assert s in msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunked_load_refuses_info_of_another_length(chunk, monkeypatch):
    """info one short and one long under a small chunk: the k-mer count passes n_info in a middle chunk (the
    copy stops there) or never reaches it; both are MTB_ERR_DB with the two counts, and name the input."""
    from metabuli_work_amd.dbbuild import HostDb
    fx, taxo, _ = fixture()
    a, b = _host_dbs(fx, taxo, "two_meetings")
    n = len(a.info)
    short = HostDb(taxo, a.diff_idx, a.info[:-1].copy(), a.split, a.taxid_list)
    long_ = HostDb(taxo, a.diff_idx, np.concatenate([a.info, a.info[:1]]), a.split, a.taxid_list)
    far_short = HostDb(taxo, a.diff_idx, a.info[: n // 2].copy(), a.split, a.taxid_list)
    monkeypatch.setenv("MTB_DECODE_CHUNK_WORDS", chunk)
    for bad, d in ((short, n - 1), (long_, n + 1), (far_short, n // 2)):
        _refused([bad, b], taxo, MTB_ERR_DB, "merge input 0", f"k-mer count {n}", f"info entries {d}")
        _refused([b, bad], taxo, MTB_ERR_DB, "merge input 1", f"k-mer count {n}", f"info entries {d}")
    # and the pair still merges afterwards
    m = _merge([a, b], taxo, int(fx["two_meetings_split_num"]))
    _assert_is(m, fx["two_meetings_diffIdx"], fx["two_meetings_info"], fx["two_meetings_split"], chunk)


# ---- many inputs ----------------------------------------------------------------------------------------
def _many_inputs(taxo, tree, n_in=64):
    """n_in inputs of 0 to about 50 k-mers over one small universe of values: two empty, several of equal
    size, values overlapping between inputs."""
    rng = np.random.default_rng(11)
    leaves = np.array([t for t, r in zip(taxo.taxid.tolist(), taxo.rank) if r == "no rank" and t != 1], np.int64)
    pool = (rng.integers(1, 21 ** 8, 40, dtype=np.uint64)[rng.integers(0, 40, 400)] << np.uint64(24)) | \
        rng.integers(0, 1 << 24, 400, dtype=np.uint64)
    sizes = rng.integers(1, 51, n_in)
    sizes[[5, 40]] = 0
    sizes[[7, 8, 9, 50, 63]] = 17
    dbs = []
    for n in sizes.tolist():
        v = rng.choice(pool, n, replace=False)
        t = rng.choice(leaves, n)
        o = np.lexsort((t, tree.sp[t], v))
        dbs.append(_db(taxo, tree, v[o], t[o]))
    return dbs


@pytest.mark.gpu
def test_sixty_four_inputs():
    """64 inputs (expectations from numpy: two are empty, which the reference cannot run); the reversed order
    gives the same bytes; chunked too."""
    _, taxo, tree = fixture()
    dbs = _many_inputs(taxo, tree)
    assert len(dbs) == 64 and sum(len(d.info) == 0 for d in dbs) == 2
    values = np.concatenate([decode_diff(d.diff_idx) for d in dbs])
    assert len(np.unique(values)) < len(values)  # values overlap between inputs
    exp = _expect(tree, dbs, 16)
    assert len(exp[1]) < len(values)
    m = _merge(dbs, taxo, 16)
    _assert_is(m, *exp, "file order")
    assert np.array_equal(m.taxid_list, np.unique(np.concatenate([d.taxid_list for d in dbs])))
    _assert_is(_merge(dbs[::-1], taxo, 16), *exp, "reversed")


@pytest.mark.gpu
def test_sixty_five_inputs_are_refused():
    """More than 64 inputs: MTB_ERR_ARG from the argument checks, before the taxonomy is built or the device
    touched (no merge ran: the phase times of the last merge stay as they were)."""
    from metabuli_work_amd.dbbuild import merge_last_ms
    _, taxo, tree = fixture()
    dbs = _many_inputs(taxo, tree, 65)
    before = merge_last_ms()
    _refused(dbs, taxo, MTB_ERR_ARG, "1 to 64 inputs")
    assert merge_last_ms() == before
