"""Group application on the host side: tests/apply_expect.py against the reference's own GroupApplier
(tests/golden/ref_group_apply.npz, made by tests/golden/make_ref_group_apply.py), its two statements of
the representative label against each other, the lineage rank the library uploads, and the refusals of
mtb_group_apply / mtb_group_apply_files that return before any device call (no GPU needed: on a machine
without one a device call would fail with MTB_ERR_HIP instead)."""
import ctypes
import json
import pathlib

import numpy as np
import pytest

from metabuli_work_amd import grouping, synth
from metabuli_work_amd._abi import MtbGroupApplyParams, MtbGroupApplyStats
from metabuli_work_amd._lib import lib
from metabuli_work_amd.dbbuild import HostDb
from tests import apply_expect as ax

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
MTB_ERR_ARG, MTB_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN / "ref_group_apply.npz")


def cases(ref):
    return [(k, int(m), float(np.float32(t))) for k, (m, t) in enumerate(zip(ref["case_mode"], ref["case_min_vote_score"]))]


def test_defaults_are_the_reference_text():
    g = json.loads((GOLDEN / "group_apply_defaults.json").read_text())["defaults"]
    p = grouping.ApplyParams.defaults()
    assert p.weight_mode == g["weightMode"]["value"] == 1
    assert np.float32(p.min_vote_score) == np.float32(g["minVoteScr"]["value"]) == np.float32(0.15)
    assert (g["taxidCol"]["value"], g["scoreCol"]["value"], g["readIdCol"]["value"]) == (3, 5, 2)
    assert grouping.apply_groups.__defaults__[1:4] == (3, 5, 2)


def test_expectation_reproduces_the_reference_files(ref):
    S = grouping.apply_constants()["slice"]
    assert bool(ref["sanitizer_clean"]) and len(cases(ref)) >= 9
    for k, mode, thr in cases(ref):
        for s in (None, S, 1, 2):
            rep, upd = ax.expected_files(ref["node_taxid"], ref["node_parent"], ref["node_rank"].tolist(),
                                         ref["tsv"].tobytes(), ref["group_map"], mode, thr, S=s)
            assert rep == ref[f"case{k}_group_rep"].tobytes(), (k, s)
            assert upd == ref[f"case{k}_updated"].tobytes(), (k, s)


def test_fixture_covers_what_it_was_designed_for(ref):
    by = {(m, t): ref[f"case{k}_group_rep"].tobytes().decode() for k, m, t in cases(ref)}
    assert {m for m, _ in by} == {0, 1, 2}
    d = by[(1, float(np.float32(0.15)))]
    assert "4\t32\n" in d and "12\t40\n" in d and "15\t0\n" in d and "17\t0\n" in d and "20\t0\n" in d
    assert "4\t31\n" in by[(1, 0.0)]               # the low scorer votes at threshold 0
    assert set(by[(1, 2.0)].split("\n")) <= {f"{g}\t0" for g in (1, 4, 8, 10, 12, 15, 17, 20, 22, 26)} | {""}
    upd = ref["case6_updated"].tobytes().decode()  # threshold 0.25 = the scores of reads 10 and 11
    assert "1\tread_11\t41\t0\t0.25\tspecies\t10\t\n" in upd   # at the threshold: votes, keeps its label
    assert "0\tread_25\t0\t0\t0\t-\t-\t-\t\n" in upd           # no group, unclassified


def random_tree(rng, n):
    ranks = ["no rank", "species", "genus", "family", "order", "class", "phylum", "superkingdom", "clade"]
    taxid, parent, rank = [1], [1], ["no rank"]
    for t in range(2, n + 2):
        taxid.append(t)
        parent.append(int(rng.integers(1, t)))
        rank.append(ranks[int(rng.integers(0, len(ranks)))])
    return taxid, parent, rank


def test_the_two_statements_agree_on_dyadic_scores(ref):
    e2i = ax.internal_ids(ref["node_taxid"], ref["node_parent"])
    tree = ax.Tree([e2i[int(t)] for t in ref["node_taxid"]], [e2i[int(p)] for p in ref["node_parent"]],
                   ref["node_rank"].tolist())
    _, labels, scores = ax.parse_tsv(ref["tsv"].tobytes())
    tax = np.array([e2i[int(x)] if x else 0 for x in labels], np.int32)
    for _, mode, thr in cases(ref):
        a = ax.apply_all(tree, ref["group_map"], tax, scores, mode, thr)
        for S in (1, 2, 3, 1024):
            b = ax.apply_all(tree, ref["group_map"], tax, scores, mode, thr, S)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    rng = np.random.default_rng(5)
    some_rep = 0
    for trial in range(60):
        taxid, parent, rank = random_tree(rng, int(rng.integers(2, 40)))
        tree = ax.Tree(taxid, parent, rank)
        m = int(rng.integers(1, 30))
        members = [(int(rng.integers(0, len(taxid) + 1)), np.float32(int(rng.integers(0, 65)) / 64.0)) for _ in range(m)]
        for mode in (0, 1, 2):
            for thr in (0.0, 0.15, 0.5):
                want = ax.rep_label_sequential(tree, members, mode, thr)
                for S in (1, 4, 1024):
                    assert ax.rep_label_device_order(tree, members, mode, thr, S) == want, (trial, mode, thr, S)
                some_rep += want != 0
    assert some_rep > 100


def designed_rank_tree():
    # 2 genus -> 3 no rank -> 4 species -> 5 no rank; 6 no rank -> 7 no rank (no ranked lineage);
    # 8 species -> 9 genus (a parent ranked lower than its child) -> 10 no rank
    taxid = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    parent = [1, 1, 2, 3, 4, 1, 6, 1, 8, 9]
    rank = ["superkingdom", "genus", "no rank", "species", "no rank", "no rank", "clade", "species", "genus", ""]
    return taxid, parent, rank


def test_lineage_rank_of_the_library_matches_the_rule():
    taxid, parent, rank = designed_rank_tree()
    want = [ax.ROOT_RANK, 8, 8, 4, 4, ax.ROOT_RANK, ax.ROOT_RANK, 4, 8, 8]
    assert ax.lineage_ranks(ax.Tree(taxid, parent, rank)).tolist() == want
    taxo = synth.Taxonomy(np.array(taxid, np.int32), np.array(parent, np.int32), rank, [f"t{t}" for t in taxid])
    assert grouping.lineage_ranks(taxo).tolist() == want
    rng = np.random.default_rng(11)
    for _ in range(5):
        taxid, parent, rank = random_tree(rng, 300)
        perm = rng.permutation(len(taxid))          # nodes.dmp rows in any order
        taxo = synth.Taxonomy(np.array(taxid, np.int32)[perm], np.array(parent, np.int32)[perm],
                              [rank[i] for i in perm], [f"t{taxid[i]}" for i in perm])
        tree = ax.Tree(taxo.taxid, taxo.parent, taxo.rank)
        assert grouping.lineage_ranks(taxo).tolist() == ax.lineage_ranks(tree).tolist()


# ---- refusals before any device call ---------------------------------------------------------------
def _apply(gm, tax, score, mode=1, flags=0, cap=None, n=None):
    taxid, parent, rank = designed_rank_tree()
    taxo = synth.Taxonomy(np.array(taxid, np.int32), np.array(parent, np.int32), rank, [f"t{t}" for t in taxid])
    hdb = HostDb(taxo)
    h = hdb.c_struct()
    par = MtbGroupApplyParams(weight_mode=mode, min_vote_score=0.15)
    gm, tax, score = np.asarray(gm, np.uint32), np.asarray(tax, np.int32), np.asarray(score, np.float32)
    n = len(tax) if n is None else n
    rg, rt = np.zeros(8, np.uint32), np.zeros(8, np.int32)
    ng = ctypes.c_uint64(8 if cap is None else cap)
    ot, oc, oa = np.zeros(max(len(tax), 1), np.int32), np.zeros(max(len(tax), 1), np.uint8), np.zeros(max(len(tax), 1), np.uint8)
    st = MtbGroupApplyStats()
    rc = lib().mtb_group_apply(0, ctypes.byref(h), ctypes.byref(par), gm.ctypes.data, tax.ctypes.data, score.ctypes.data,
                               n, flags, rg.ctypes.data, rt.ctypes.data, ctypes.byref(ng), ot.ctypes.data, oc.ctypes.data,
                               oa.ctypes.data, ctypes.byref(st))
    return rc, lib().mtb_last_error().decode()


def test_apply_refuses_on_the_host():
    ok = ([0, 1, 1], [4, 0], [0.5, 0.0])
    for mode in (-1, 3):
        rc, msg = _apply(*ok, mode=mode)
        assert rc == MTB_ERR_ARG and "weight_mode" in msg
    rc, msg = _apply(*ok, flags=2)
    assert rc == MTB_ERR_ARG and "MTB_INPUT_DEVICE" in msg
    rc, msg = _apply([0, 1, 1, 1], [4, 11, 12], [0.5, 0.5, 0.5])   # 11: past the taxonomy; named first
    assert rc == MTB_ERR_ARG and "read 2" in msg and "11" in msg
    rc, msg = _apply([0, 1, 1], [4, -3], [0.5, 0.5])
    assert rc == MTB_ERR_ARG and "read 2" in msg
    rc, msg = _apply([0, 1, 0xFFFFFFFF], [4, 4], [0.5, 0.5])
    assert rc == MTB_ERR_ARG and "read 2" in msg and "2^32 - 1" in msg
    rc, msg = _apply(*ok, n=0xFFFFFFFF)
    assert rc == MTB_ERR_ARG and "reads" in msg


def _write_case(tmp_path, ref, tsv=None, group_map=None, groups=None, nodes=None):
    d = tmp_path / "in"
    (d / "taxonomy").mkdir(parents=True, exist_ok=True)
    (d / "taxonomy" / "nodes.dmp").write_bytes(ref["nodes_dmp"].tobytes() if nodes is None else nodes)
    (d / "taxonomy" / "names.dmp").write_bytes(ref["names_dmp"].tobytes())
    (d / "taxonomy" / "merged.dmp").write_bytes(b"")
    (d / "classifications.tsv").write_bytes(ref["tsv"].tobytes() if tsv is None else tsv)
    gm = ref["group_map"] if group_map is None else group_map
    (d / "groupMap").write_text("".join(f"{i}\t{g}\n" for i, g in enumerate(np.asarray(gm)[1:].tolist(), 1)))
    (d / "groups").write_bytes(ref["groups"].tobytes() if groups is None else groups)
    return d


def _apply_files(d, out, mode=1, cols=(3, 5, 2), groups=True):
    out.mkdir(exist_ok=True)
    par = MtbGroupApplyParams(weight_mode=mode, min_vote_score=0.15)
    st = MtbGroupApplyStats()
    rc = lib().mtb_group_apply_files(str(d / "groups").encode() if groups else None, str(d / "groupMap").encode(),
                                     str(d / "taxonomy").encode(), str(d / "classifications.tsv").encode(),
                                     str(out).encode(), ctypes.byref(par), cols[0], cols[1], cols[2], 0, ctypes.byref(st))
    return rc, lib().mtb_last_error().decode()


def test_apply_files_refuses_on_the_host(tmp_path, ref):
    out = tmp_path / "out"
    d = _write_case(tmp_path, ref)
    rc, msg = _apply_files(d, out, mode=3)
    assert rc == MTB_ERR_ARG and "weight_mode" in msg
    rc, msg = _apply_files(d, out, cols=(3, 9, 2))
    assert rc == MTB_ERR_ARG and "column 9" in msg
    rc, msg = _apply_files(d, out, cols=(0, 5, 2))
    assert rc == MTB_ERR_ARG
    d = _write_case(tmp_path, ref, group_map=ref["group_map"][:-1])
    rc, msg = _apply_files(d, out, groups=False)
    assert rc == MTB_ERR_ARG and "groupMap holds" in msg
    tsv = ref["tsv"].tobytes().replace(b"read_3\t32\t", b"read_3\t999\t")
    rc, msg = _apply_files(_write_case(tmp_path, ref, tsv=tsv), out)
    assert rc == MTB_ERR_ARG and "read 3" in msg and "read_3" in msg and "999" in msg
    gm = ref["group_map"].copy()
    gm[5] = 1                                               # groupMap moves read 5 into group 1; groups does not
    rc, msg = _apply_files(_write_case(tmp_path, ref, group_map=gm), out)
    assert rc == MTB_ERR_ARG and "groupMap" in msg
    d = _write_case(tmp_path, ref)
    (d / "groupMap").write_text("".join(f"{i}\t{4294967295 if i == 2 else 0}\n" for i in range(1, len(ref["group_map"]))))
    rc, msg = _apply_files(d, out, groups=False)
    assert rc == MTB_ERR_ARG and "read 2" in msg and "4294967295" in msg
    nodes = ref["nodes_dmp"].tobytes().split(b"\n")
    nodes = b"\n".join([nodes[1], nodes[0]] + nodes[2:])    # "10 | 1" first: taxID 10 would be internal 1
    rc, msg = _apply_files(_write_case(tmp_path, ref, nodes=nodes), out)
    assert rc == MTB_ERR_UNSUPPORTED and "root" in msg
    assert not (out / "groupRep").exists() and not (out / "updated_classifications.tsv").exists()
