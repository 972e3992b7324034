"""Group application on the device (mtb_group_apply, mtb_group_apply_files) against tests/apply_expect.py:
representatives, per-read labels and flags, per-label sums and the two files, all compared exactly."""
import ctypes
import pathlib

import numpy as np
import pytest
import torch  # before the library is loaded, as in test_gpu_build.py: the device-resident inputs are tensors

from metabuli_work_amd import grouping, synth
from metabuli_work_amd._abi import MTB_RETRY, MtbGroupApplyParams, MtbGroupApplyStats
from metabuli_work_amd._lib import lib
from metabuli_work_amd.dbbuild import HostDb
from metabuli_work_amd.grouping import ApplyParams
from tests import apply_expect as ax

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
CONST = grouping.apply_constants()
S, THREAD, WAVE = CONST["slice"], CONST["thread_labels"], CONST["wave_labels"]


def taxo_of(taxid, parent, rank):
    return synth.Taxonomy(np.array(taxid, np.int32), np.array(parent, np.int32), list(rank), [f"t{t}" for t in taxid])


def run_and_check(tree, taxo, gm, tax, score, mode, thr, device_arrays=False):
    """apply_groups_arrays against the device-order expectation; returns the expectation."""
    gm, tax = np.asarray(gm, np.uint32), np.asarray(tax, np.int32)
    score = None if score is None else np.asarray(score, np.float32)
    want = ax.apply_all(tree, gm, tax, score, mode, thr, S)
    par = ApplyParams(mode, thr)
    if device_arrays:
        t = lambda a, dt: None if a is None else torch.from_numpy(a.view(dt) if a.dtype == np.uint32 else a).cuda()
        got = grouping.apply_groups_arrays(t(gm, np.int32), t(tax, np.int32), t(score, np.float32), taxo, par)
        assert all(x.is_cuda for x in got[:5])
        got = [x.cpu().numpy() for x in got[:5]] + [got[5]]
        got[0] = got[0].view(np.uint32)
    else:
        got = grouping.apply_groups_arrays(gm, tax, score, taxo, par)
    for name, g, w in zip(("rep_groups", "rep_tax", "out_tax", "out_classified", "applied"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, g, w)
    st = got[5]
    assert st["reads"] == len(tax) and st["groups"] == len(want[0])
    assert st["groups_with_rep"] == int((want[1] != 0).sum()) and st["applied"] == int(want[4].sum())
    sc = np.ones(len(tax), np.float32) if score is None else score
    votes = (gm[1:] != 0) & (tax != 0) & ((mode == 0) | (sc >= np.float32(thr)))
    assert st["voting_reads"] == int(votes.sum())
    return want


# ---- the reference fixture ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN / "ref_group_apply.npz")


@pytest.fixture(scope="module")
def fixture_arrays(ref):
    e2i = ax.internal_ids(ref["node_taxid"], ref["node_parent"])
    taxid = [e2i[int(t)] for t in ref["node_taxid"]]
    parent = [e2i[int(p)] for p in ref["node_parent"]]
    rank = ref["node_rank"].tolist()
    _, labels, scores = ax.parse_tsv(ref["tsv"].tobytes())
    tax = np.array([e2i[int(x)] if x else 0 for x in labels], np.int32)
    return ax.Tree(taxid, parent, rank), taxo_of(taxid, parent, rank), tax, scores, e2i


def ref_cases(ref):
    return [(k, int(m), float(np.float32(t))) for k, (m, t) in enumerate(zip(ref["case_mode"], ref["case_min_vote_score"]))]


@pytest.mark.gpu
@pytest.mark.parametrize("device_arrays", [False, True])
def test_fixture_cases_through_arrays(ref, fixture_arrays, device_arrays):
    tree, taxo, tax, scores, e2i = fixture_arrays
    i2e = {i: e for e, i in e2i.items()}
    i2e[0] = 0
    for k, mode, thr in ref_cases(ref):
        groups, reps, *_ = run_and_check(tree, taxo, ref["group_map"], tax, scores, mode, thr, device_arrays)
        text = "".join(f"{g}\t{i2e[int(t)]}\n" for g, t in zip(groups.tolist(), reps.tolist()))
        assert text.encode() == ref[f"case{k}_group_rep"].tobytes(), k


def _write_inputs(d, ref):
    (d / "taxonomy").mkdir(parents=True)
    (d / "taxonomy" / "nodes.dmp").write_bytes(ref["nodes_dmp"].tobytes())
    (d / "taxonomy" / "names.dmp").write_bytes(ref["names_dmp"].tobytes())
    (d / "taxonomy" / "merged.dmp").write_bytes(b"")
    (d / "classifications.tsv").write_bytes(ref["tsv"].tobytes())
    (d / "groups").write_bytes(ref["groups"].tobytes())
    (d / "groupMap").write_text("".join(f"{i}\t{g}\n" for i, g in enumerate(ref["group_map"][1:].tolist(), 1)))


@pytest.mark.gpu
def test_fixture_cases_through_files(tmp_path, ref):
    d = tmp_path / "in"
    _write_inputs(d, ref)
    for k, mode, thr in ref_cases(ref):
        out = tmp_path / f"out{k}"
        st = grouping.apply_groups(d, d / "taxonomy", d / "classifications.tsv", out, ApplyParams(mode, thr))
        assert (out / "groupRep").read_bytes() == ref[f"case{k}_group_rep"].tobytes(), k
        assert (out / "updated_classifications.tsv").read_bytes() == ref[f"case{k}_updated"].tobytes(), k
        assert st["reads"] == len(ref["group_map"]) - 1 and st["groups"] == 10
    # other columns: the name first, the score last
    rows = [ln.split("\t") for ln in ref["tsv"].tobytes().decode().split("\n") if ln and ln[0] != "#"]
    alt = "".join(f"{r[1]}\t{r[2]}\tx\t{r[4]}\n" for r in rows).encode()
    (d / "alt.tsv").write_bytes(alt)
    grouping.apply_groups(d, d / "taxonomy", d / "alt.tsv", tmp_path / "alt", ApplyParams(1, 0.15), taxid_col=2,
                          score_col=4, read_id_col=1)
    assert (tmp_path / "alt" / "updated_classifications.tsv").read_bytes() == ref["case1_updated"].tobytes()


# ---- label counts at every path threshold ---------------------------------------------------------------
def generated_tree(n_families=6, genera=7, species=12):
    taxid, parent, rank = [1, 2], [1, 1], ["no rank", "superkingdom"]
    sp = []
    for f in range(n_families):
        fam = len(taxid) + 1
        taxid.append(fam); parent.append(2); rank.append("family")
        for g in range(genera):
            gen = len(taxid) + 1
            taxid.append(gen); parent.append(fam); rank.append("genus" if g % 3 else "no rank")
            for s in range(species):
                t = len(taxid) + 1
                taxid.append(t); parent.append(gen); rank.append("species")
                sp.append(t)
    return taxid, parent, rank, sp


@pytest.mark.gpu
def test_label_counts_on_each_side_of_every_threshold():
    taxid, parent, rank, species = generated_tree()
    tree, taxo = ax.Tree(taxid, parent, rank), taxo_of(taxid, parent, rank)
    assert len(species) > 3 * WAVE
    counts = sorted({1, 2, THREAD - 1, THREAD, THREAD + 1, WAVE - 1, WAVE, WAVE + 1, 3 * WAVE + 5})
    rng = np.random.default_rng(9)
    gm, tax, score = [0], [], []
    for rep in range(3):           # three weightings per count: flat, one heavy genus, one heavy species
        for m in counts:
            gid = len(gm)
            pool = species if rep != 1 else species[:max(m, 14)]
            labs = rng.choice(pool, m, replace=False)
            if m > 2 and rep == 0:
                labs[0] = tree.parent[int(labs[1])]      # a label that is an ancestor of another
            for j, lab in enumerate(labs.tolist()):
                for _ in range(int(rng.integers(1, 4))):
                    w = int(rng.integers(1, 9))
                    if rep == 2 and j == 0:
                        w = 64
                    gm.append(gid); tax.append(lab); score.append(min(w * m if rep == 2 and j == 0 else w, 64 * 64) / 64.0)
            gm.append(gid); tax.append(0); score.append(0.5)
    order = rng.permutation(len(tax))                    # members of a group are not adjacent
    gm = np.array([0] + [gm[1:][i] for i in order], np.uint32)
    tax, score = np.array(tax, np.int32)[order], np.array(score, np.float32)[order]
    for mode in (1, 2):
        groups, reps, *_ = run_and_check(tree, taxo, gm, tax, score, mode, 0.0)
        assert len(groups) == 3 * len(counts) and 5 < (reps != 0).sum()
        assert len({tree.rank[int(t)] for t in reps if t}) >= 2       # species and LCAs both win somewhere


@pytest.mark.gpu
def test_label_sums_follow_the_slice_order():
    taxid, parent, rank, species = generated_tree(2, 2, 3)
    tree, taxo = ax.Tree(taxid, parent, rank), taxo_of(taxid, parent, rank)
    rng = np.random.default_rng(21)
    gm, tax = [0], []
    for k, run in enumerate((S - 1, S, S + 1, 2 * S + 1)):
        gid = len(gm)
        gm += [gid] * (run + 7)
        tax += [species[0]] * run + [species[1]] * 4 + [species[5]] * 3
    order = rng.permutation(len(tax))
    gm = np.array([0] + [gm[1:][i] for i in order], np.uint32)
    tax = np.array(tax, np.int32)[order]
    # not dyadic and spread over twelve decades: a double sum of them rounds, so its order shows
    score = (rng.random(len(tax)) * 10.0 ** (-rng.integers(0, 12, len(tax)).astype(np.float64))).astype(np.float32)
    differs = 0
    for mode in (1, 2):
        g, lab, w = grouping.apply_label_sums(gm, tax, score, taxo, ApplyParams(mode, 0.0))
        members = ax.group_members(gm)
        assert g.tolist() == sorted(g.tolist()) and len(g) == 12
        for gid in sorted(members):
            mem = [(int(tax[r]), score[r]) for r in members[gid]]
            want = ax.label_sums(mem, mode, 0.0, S)
            plain = ax.label_sums(mem, mode, 0.0, 1 << 30)
            sel = g == gid
            assert lab[sel].tolist() == sorted(want)
            assert [float(x).hex() for x in w[sel]] == [want[v].hex() for v in sorted(want)], (mode, gid)
            differs += any(want[v] != plain[v] for v in want)
        run_and_check(tree, taxo, gm, tax, score, mode, 0.0)
    assert differs >= 1          # a run past one slice does not sum as the plain sequential sum does


# ---- ratio edges (dyadic scores: every share is exact) ---------------------------------------------------
@pytest.fixture(scope="module")
def edge_tree():
    # 2 superkingdom; 3 genus: species 4, 5; 6 genus: species 7 (strain 8), 9; 10 no rank: 11 no rank; 12 superkingdom: 13 species
    taxid = [1, 2, 3, 5, 4, 6, 7, 8, 9, 10, 11, 12, 13]
    parent = [1, 1, 2, 3, 3, 2, 6, 7, 6, 1, 10, 1, 12]
    rank = ["no rank", "superkingdom", "genus", "species", "species", "genus", "species", "no rank", "species", "no rank",
            "no rank", "superkingdom", "species"]
    return ax.Tree(taxid, parent, rank), taxo_of(taxid, parent, rank)


EDGES = {  # name: (members (label, score x 64), mode, threshold, representative)
    "siblings_at_half": ([(5, 16), (4, 16)], 1, 0.0, 4),
    "half_against_just_below": ([(5, 32), (4, 31), (7, 1)], 1, 0.0, 5),
    "just_below_half_falls_to_the_genus": ([(5, 31), (4, 31), (7, 2)], 1, 0.0, 3),
    "ancestor_label": ([(8, 40), (7, 8), (0, 48)], 1, 0.0, 7),
    "ancestor_label_below_half": ([(8, 8), (6, 4), (4, 8)], 1, 0.0, 6),
    "three_labels_two_lcas": ([(4, 16), (7, 16), (9, 16)], 1, 0.0, 6),
    "three_labels_top_lca": ([(4, 16), (5, 8), (7, 16), (9, 8), (13, 2)], 1, 0.0, 2),
    "total_weight_zero": ([(4, 0), (5, 0)], 1, 0.0, 0),
    "all_votes_on_the_root": ([(1, 32), (1, 8)], 1, 0.0, 0),
    "resolves_to_the_root": ([(4, 16), (11, 16), (13, 16)], 1, 0.0, 0),
    "unranked_lineage_loses_to_a_rank": ([(11, 32), (13, 32)], 1, 0.0, 13),
    "unranked_lineage_alone": ([(11, 32), (10, 8)], 1, 0.0, 10),
    "mode2_squares": ([(4, 48), (5, 32), (5, 32)], 2, 0.0, 4),
    "mode0_counts": ([(4, 48), (5, 1), (5, 1)], 0, 0.0, 5),
    "threshold_drops_voters": ([(4, 8), (4, 8), (5, 10)], 1, 10 / 64, 5),
}


@pytest.mark.gpu
def test_ratio_edges(edge_tree):
    tree, taxo = edge_tree
    for mode in (0, 1, 2):
        names = [n for n in EDGES if EDGES[n][1] == mode]
        for thr in sorted({EDGES[n][2] for n in names}):
            gm, tax, score, want = [0], [], [], {}
            for n in names:
                if EDGES[n][2] != thr:
                    continue
                gid = len(gm)
                for lab, s64 in EDGES[n][0]:
                    gm.append(gid); tax.append(lab); score.append(s64 / 64.0)
                want[gid] = (n, EDGES[n][3])
            groups, reps, *_ = run_and_check(tree, taxo, gm, tax, score, mode, thr)
            for g, t in zip(groups.tolist(), reps.tolist()):
                assert t == want[g][1], want[g][0]
                mem = [(tax[r], np.float32(score[r])) for r in ax.group_members(gm)[g]]
                assert ax.rep_label_sequential(tree, mem, mode, thr) == t, want[g][0]


@pytest.mark.gpu
def test_per_read_rule_around_the_threshold(edge_tree):
    tree, taxo = edge_tree
    thr = np.float32(0.15)
    below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
    gm = [0] + [1] * 7 + [0, 0]
    tax = [4, 4, 5, 5, 5, 0, 0, 5, 0]
    score = [0.9, 0.8, below, thr, above, 0.9, 0.0, below, 0.0]
    for mode in (0, 1, 2):
        groups, reps, out_tax, cls, app = run_and_check(tree, taxo, gm, tax, score, mode, float(thr))
        assert reps.tolist() == ([4] if mode else [5])
        if mode == 0:
            assert out_tax[:7].tolist() == [5] * 7 and app[:7].all()
        else:       # below the threshold and label 0 take the representative; at and above keep theirs
            assert out_tax.tolist() == [4, 4, 4, 5, 5, 4, 4, 5, 0]
            assert app.tolist() == [False, False, True, False, False, True, True, False, False]
        assert cls.tolist() == [True] * 8 + [False]


@pytest.mark.gpu
def test_sparse_large_group_ids_and_tiny_inputs(edge_tree):
    tree, taxo = edge_tree
    ids = [5, 70000, 2 ** 31 + 3, 2 ** 32 - 2]
    gm = [0] + [ids[i % 4] for i in range(23)] + [0]
    tax = [[4, 5, 7, 9][(i * 7) % 4] if i % 5 else 0 for i in range(24)]
    score = [((i * 13) % 64) / 64.0 for i in range(24)]
    groups, *_ = run_and_check(tree, taxo, gm, tax, score, 1, 0.15)
    assert groups.tolist() == ids
    run_and_check(tree, taxo, gm, tax, score, 1, 0.15, device_arrays=True)
    run_and_check(tree, taxo, [0, 9], [4], [0.5], 1, 0.15)                 # one read in a group
    run_and_check(tree, taxo, [0, 0], [4], [0.5], 1, 0.15)                 # one read, no group
    run_and_check(tree, taxo, [0], [], [], 1, 0.15)                        # no read
    groups, *_ = run_and_check(tree, taxo, [0, 0, 0, 0], [4, 0, 5], None, 0, 0.15)   # no group at all, mode 0 without scores
    assert len(groups) == 0


@pytest.mark.gpu
def test_short_rep_capacity_is_a_retry(edge_tree):
    _, taxo = edge_tree
    hdb = HostDb(taxo)
    h = hdb.c_struct()
    par = MtbGroupApplyParams(weight_mode=1, min_vote_score=0.15)
    gm, tax, score = np.array([0, 3, 1, 3, 2], np.uint32), np.array([4, 5, 4, 7], np.int32), np.full(4, 0.5, np.float32)
    ot, oc, oa = np.zeros(4, np.int32), np.zeros(4, np.uint8), np.zeros(4, np.uint8)
    st = MtbGroupApplyStats()
    for cap in (0, 2, 3):
        rg, rt = np.full(4, 77, np.uint32), np.full(4, 77, np.int32)
        ng = ctypes.c_uint64(cap)
        rc = lib().mtb_group_apply(0, ctypes.byref(h), ctypes.byref(par), gm.ctypes.data, tax.ctypes.data, score.ctypes.data,
                                   4, 0, rg.ctypes.data, rt.ctypes.data, ctypes.byref(ng), ot.ctypes.data, oc.ctypes.data,
                                   oa.ctypes.data, ctypes.byref(st))
        assert ng.value == 3 and rc == (0 if cap >= 3 else MTB_RETRY), lib().mtb_last_error().decode()
        assert rg.tolist() == ([1, 2, 3, 77] if cap >= 3 else [77] * 4)
        assert rt.tolist() == ([5, 7, 4, 77] if cap >= 3 else [77] * 4)


@pytest.mark.gpu
def test_unknown_label_on_the_device_is_refused(edge_tree):
    _, taxo = edge_tree
    gm = torch.tensor([0, 1, 1, 1], dtype=torch.int32).cuda()
    tax = torch.tensor([4, 99, 77], dtype=torch.int32).cuda()
    sc = torch.full((3,), 0.5).cuda()
    with pytest.raises(Exception, match="read 2"):
        grouping.apply_groups_arrays(gm, tax, sc, taxo, ApplyParams(1, 0.15))


# ---- end to end ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_to_end_group_reads_then_apply_groups(tmp_path):
    """Pairs of two species built as test_group_gpu.py builds its reads, through group_reads; a hand-made
    classification TSV (a fifth unclassified, some scored low, a few of the other species); apply_groups:
    both files equal the expectation's."""
    from metabuli_work_amd.grouping import GroupParams, group_reads
    from tests.test_group_gpu import _fastq, _synthetic_pairs

    n, glen, seed = 3000, 30000, 3
    s1, o1, s2, o2 = _synthetic_pairs(n, glen, seed)
    rng = np.random.default_rng(seed)
    rng.integers(0, 4, (3, glen))
    genome = rng.integers(0, 3, n)                    # the genome each pair was drawn from
    (tmp_path / "r1.fq").write_bytes(_fastq(s1, o1))
    (tmp_path / "r2.fq").write_bytes(_fastq(s2, o2))
    gm, _ = group_reads(tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / "grp", GroupParams())
    assert len(np.unique(gm[gm != 0])) >= 2 and (gm != 0).sum() > n // 2

    nodes = [(1, 1, "no rank"), (2, 1, "superkingdom"), (30, 2, "genus"), (301, 30, "species"), (302, 30, "species"),
             (3011, 301, "no rank")]
    tdir = tmp_path / "taxonomy"
    taxo = synth.Taxonomy(np.array([t for t, _, _ in nodes], np.int32), np.array([p for _, p, _ in nodes], np.int32),
                          [r for _, _, r in nodes], [f"taxon_{t}" for t, _, _ in nodes])
    taxo.write_dmp(str(tdir))
    r2 = np.random.default_rng(17)
    truth = np.where(genome == 2, 302, np.where(genome == 1, 3011, 301))
    label = np.where(r2.random(n) < 0.2, 0, np.where(r2.random(n) < 0.05, 302, truth))
    score = (r2.integers(0, 65, n) / 64.0).astype(np.float32)
    rows = ["#is_classified\tname\ttaxID\tquery_length\tscore\trank\ttaxID:match_count\n"]
    rows += [f"{int(l != 0)}\tr{i}\t{l}\t300\t{'%.9g' % float(s)}\t-\t-\n" for i, (l, s) in enumerate(zip(label.tolist(), score))]
    tsv = "".join(rows).encode()
    (tmp_path / "cls.tsv").write_bytes(tsv)
    for mode, thr in ((1, 0.15), (0, 0.15), (2, 0.5)):
        out = tmp_path / f"out{mode}"
        st = grouping.apply_groups(tmp_path / "grp", tdir, tmp_path / "cls.tsv", out, ApplyParams(mode, thr))
        rep, upd = ax.expected_files(taxo.taxid, taxo.parent, taxo.rank, tsv, gm, mode, thr, S)
        assert (out / "groupRep").read_bytes() == rep
        assert (out / "updated_classifications.tsv").read_bytes() == upd
        assert st["applied"] > 100 and st["groups_with_rep"] >= 2
