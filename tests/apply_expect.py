"""Group application in plain Python and numpy: what mtb_group_apply and mtb_group_apply_files must
produce (include/mtb_gpu.h, "group application"). Two statements of the representative label:
rep_label_sequential follows the published weightedMajorityLCA vote by vote in member order;
rep_label_device_order takes the sums in the order the device contract fixes. They agree whenever every
sum is exact (dyadic scores)."""
import numpy as np

ROOT_RANK = 2 ** 31 - 1
# MMseqs2 NcbiRanks (findRankIndex) plus "domain" (TaxonomyWrapper::findRankIndex2), restated
RANK_INDEX = {"forma": 1, "varietas": 2, "subspecies": 3, "species": 4, "species subgroup": 5, "species group": 6,
              "subgenus": 7, "genus": 8, "subtribe": 9, "tribe": 10, "subfamily": 11, "family": 12, "superfamily": 13,
              "parvorder": 14, "infraorder": 15, "suborder": 16, "order": 17, "superorder": 18, "infraclass": 19,
              "subclass": 20, "class": 21, "superclass": 22, "subphylum": 23, "phylum": 24, "superphylum": 25,
              "subkingdom": 26, "kingdom": 27, "superkingdom": 28, "domain": 28}


class Tree:
    """A taxonomy by taxID: parent and rank of every node; the root is taxID 1."""

    def __init__(self, taxid, parent, rank):
        self.taxid = [int(t) for t in taxid]
        self.parent = {int(t): int(p) for t, p in zip(taxid, parent)}
        self.rank = {int(t): r for t, r in zip(taxid, rank)}
        self.parent[1] = 1
        self._lineage = {}

    def lineage(self, t):
        """t, its parent, ..., the root."""
        if t not in self._lineage:
            out = [t]
            while out[-1] != 1:
                out.append(self.parent[out[-1]])
            self._lineage[t] = out
        return self._lineage[t]

    def lineage_rank(self, t):
        """The rank index of the first node with an index > 0 from t towards the root, the root itself
        never looked at; ROOT_RANK when there is none."""
        for a in self.lineage(t):
            if a == 1:
                break
            r = RANK_INDEX.get(self.rank[a], -1)
            if r > 0:
                return r
        return ROOT_RANK

    def lca(self, a, b):
        la = set(self.lineage(a))
        for x in self.lineage(b):
            if x in la:
                return x
        raise ValueError("no common ancestor")

    def in_clade(self, v, c):
        return c in self.lineage(v)


def lineage_ranks(tree):
    return np.array([tree.lineage_rank(t) for t in tree.taxid], np.int64)


def vote_weight(score, mode):
    """float32 score -> the vote's weight as the reference forms it (a float), widened to double."""
    s = np.float32(score)
    if mode == 0:
        return 1.0
    return float(s) if mode == 1 else float(np.float32(s * s))


def votes(members, mode, thr):
    """members: (label, score) in member order -> the (label, weight) of those that vote."""
    thr = np.float32(thr)
    out = []
    for lab, sc in members:
        if lab != 0 and (mode == 0 or np.float32(sc) >= thr):
            out.append((int(lab), vote_weight(sc, mode)))
    return out


def _choose(tree, cand, total):
    """cand: {taxID: weight} of the candidates -> the winner, or 0."""
    if total == 0:
        return 0
    best = None
    for t in sorted(cand):
        ratio = cand[t] / total
        if not ratio >= 0.5:
            continue
        r = tree.lineage_rank(t)
        if best is None or r < best[0] or (r == best[0] and ratio > best[1]):
            best = (r, ratio, t)
    return best[2] if best else 0


def rep_label_sequential(tree, members, mode, thr):
    """weightedMajorityLCA(votes, 0.5) vote by vote: every vote adds its weight to its node and every
    ancestor; a node is a candidate when it is a vote's label or got weight through two children.
    Returns the representative (0: none; 1, the root, also becomes none)."""
    weight, children, candidate = {}, {}, set()
    total = 0.0
    for lab, w in votes(members, mode, thr):
        total += w
        prev = None
        for a in tree.lineage(lab):
            weight[a] = weight.get(a, 0.0) + w
            if prev is None:
                candidate.add(a)
            else:
                children.setdefault(a, set()).add(prev)
                if len(children[a]) >= 2:
                    candidate.add(a)
            prev = a
    t = _choose(tree, {c: weight[c] for c in candidate}, total)
    return 0 if t in (0, 1) else t


def label_sums(members, mode, thr, S):
    """{label: W} in the device's order: per label its voting members in member order, slices of S each
    summed from 0.0, the slice sums added in slice order."""
    per = {}
    for lab, w in votes(members, mode, thr):
        per.setdefault(lab, []).append(w)
    out = {}
    for lab, ws in per.items():
        tot = 0.0
        for i in range(0, len(ws), S):
            s = 0.0
            for w in ws[i:i + S]:
                s += w
            tot += s
        out[lab] = tot
    return out


def rep_label_device_order(tree, members, mode, thr, S):
    """The same representative from the per-label sums: candidates = the labels and the LCAs among them,
    a candidate's weight = the sum of W over the labels in its clade ascending by taxID, the total the
    same over all labels."""
    W = label_sums(members, mode, thr, S)
    labs = sorted(W)
    total = 0.0
    for v in labs:
        total += W[v]
    cands = set(labs)
    for i, a in enumerate(labs):
        for b in labs[i + 1:]:
            cands.add(tree.lca(a, b))
    cand = {}
    for c in cands:
        s = 0.0
        for v in labs:
            if tree.in_clade(v, c):
                s += W[v]
        cand[c] = s
    t = _choose(tree, cand, total)
    return 0 if t in (0, 1) else t


def group_members(group_map):
    """{group ID: 0-based read indices ascending} of a groupMap (entry 0 unused, ID 0 = no group)."""
    gm = np.asarray(group_map, np.uint32)[1:]
    out = {}
    for r in np.nonzero(gm)[0].tolist():
        out.setdefault(int(gm[r]), []).append(r)
    return out


def apply_all(tree, group_map, tax, score, mode, thr, S=None):
    """(rep_groups, rep_tax, out_tax, out_classified, applied) of a whole call; S None: sequential sums."""
    gm = np.asarray(group_map, np.uint32)
    n = len(gm) - 1
    score = np.ones(n, np.float32) if score is None else np.asarray(score, np.float32)
    thr32 = np.float32(thr)
    reps = {}
    for g, rs in group_members(gm).items():
        mem = [(int(tax[r]), score[r]) for r in rs]
        reps[g] = (rep_label_sequential(tree, mem, mode, thr) if S is None
                   else rep_label_device_order(tree, mem, mode, thr, S))
    out_tax, cls, app = np.zeros(n, np.int32), np.zeros(n, bool), np.zeros(n, bool)
    for r in range(n):
        rep = reps.get(int(gm[r + 1]), 0)
        t = int(tax[r])
        a = rep != 0 and (mode == 0 or t == 0 or bool(score[r] < thr32))
        out_tax[r] = rep if a else t
        cls[r] = rep != 0 or t != 0
        app[r] = a
    groups = np.array(sorted(reps), np.uint32)
    return groups, np.array([reps[int(g)] for g in groups], np.int32), out_tax, cls, app


# ---- the files ---------------------------------------------------------------------------------------
def internal_ids(node_taxid, node_parent):
    """{external: internal} as TaxonomyWrapper(names, nodes, merged, true) numbers nodes.dmp: from 1, in
    order of first appearance, a row's taxID before its parent's."""
    out = {}
    for t, p in zip(node_taxid, node_parent):
        for x in (int(t), int(p)):
            if x not in out:
                out[x] = len(out) + 1
    return out


def parse_tsv(text, taxid_col=3, score_col=5, read_id_col=2, uniform=False):
    """loadOrgResult: (names, labels, scores) of a classification TSV (bytes)."""
    names, labels, scores = [], [], []
    for line in text.decode().split("\n"):
        if not line or line[0] == "#":
            continue
        col = line.split("\t")
        names.append(col[read_id_col - 1])
        labels.append(int(col[taxid_col - 1]))
        scores.append(np.float32(1.0) if uniform else np.float32(float(col[score_col - 1])))
    return names, np.array(labels, np.int64), np.array(scores, np.float32)


def expected_files(node_taxid, node_parent, node_rank, tsv, group_map, mode, thr, S=None, cols=(3, 5, 2)):
    """(groupRep bytes with groups ascending, updated_classifications.tsv bytes)."""
    e2i = internal_ids(node_taxid, node_parent)
    i2e = {i: e for e, i in e2i.items()}
    i2e[0] = 0
    tree = Tree([e2i[int(t)] for t in node_taxid], [e2i[int(p)] for p in node_parent], node_rank)
    uniform = mode == 0 or cols[1] < 1
    names, labels, scores = parse_tsv(tsv, cols[0], cols[1], cols[2], uniform)
    tax = np.array([e2i[int(x)] if x else 0 for x in labels], np.int32)
    groups, reps, out_tax, cls, app = apply_all(tree, group_map, tax, scores, mode, thr, S)
    rep_text = "".join(f"{g}\t{i2e[int(t)]}\n" for g, t in zip(groups.tolist(), reps.tolist()))
    gm = np.asarray(group_map, np.uint32)
    rows = ["#is_classified\tname\ttaxID\tquery_length\tscore\trank\tgroup\ttaxID:match_count\n"]
    for r, name in enumerate(names):
        grp = str(int(gm[r + 1])) if gm[r + 1] else "-"
        sc = "%g" % float(scores[r])
        if cls[r]:
            rows.append(f"1\t{name}\t{i2e[int(out_tax[r])]}\t0\t{sc}\t{tree.rank[int(out_tax[r])]}\t{grp}\t\n")
        else:
            rows.append(f"0\t{name}\t0\t0\t{sc}\t-\t{grp}\t-\t\n")
    return rep_text.encode(), "".join(rows).encode()
