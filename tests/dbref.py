"""Plain numpy / Python restatements shared by the DB-builder and merge tests (expected values never
come from the code under test): the diffIdx decode and word count, and the synthetic taxonomy's
species and LCA by parent walks."""
import numpy as np


def decode_diff(diff):
    """getNextTargetKmer over a whole diffIdx: the k-mer values."""
    w = np.asarray(diff, np.uint64)
    if len(w) == 0:
        return np.zeros(0, np.uint64)
    term = (w >> np.uint64(15)).astype(bool)
    ends = np.flatnonzero(term)
    gid = np.concatenate([[0], np.cumsum(term)[:-1]]).astype(np.int64)
    sh = (15 * (ends[gid] - np.arange(len(w)))).astype(np.uint64)
    delta = np.zeros(len(ends), np.uint64)
    np.add.at(delta, gid, (w & np.uint64(0x7FFF)) << sh)
    return np.cumsum(delta, dtype=np.uint64)


def diff_words(values):
    """Words getDiffIdx writes per k-mer."""
    v = np.asarray(values, np.uint64)
    d = np.diff(np.concatenate([[np.uint64(0)], v]).astype(np.uint64))
    n = np.ones(len(v), np.int64)
    for k in range(1, 5):
        n += (d >> np.uint64(15 * k)) > 0
    return n


# MMseqs2's NcbiRanks as far as the synthetic trees use them ("no rank", "accession": not in the
# table, findRankIndex gives -1)
_RANK_INDEX = {"subspecies": 3, "species": 4, "genus": 8, "family": 12, "order": 17, "class": 21, "phylum": 24,
               "superkingdom": 28}


class Tree:
    """Species and LCA of the synthetic taxonomy, by parent walks."""

    def __init__(self, taxo):
        self.parent = dict(zip(taxo.taxid.tolist(), taxo.parent.tolist()))
        self.rank = dict(zip(taxo.taxid.tolist(), taxo.rank))
        self.depth = {}
        for t in self.parent:
            d, x = 0, t
            while x != 1:
                x = self.parent[x]
                d += 1
            self.depth[t] = d
        self.sp = np.zeros(int(taxo.taxid.max()) + 1, np.int64)
        for t in self.parent:
            x = t
            while x != 1 and self.rank[x] != "species":
                x = self.parent[x]
            self.sp[t] = x if self.rank[x] == "species" else 0

    def lca(self, a, b):
        while a != b:
            da, db = self.depth[a], self.depth[b]
            if da >= db:
                a = self.parent[a]
            if db >= da:
                b = self.parent[b]
        return a

    def species_of(self, t):
        """getTaxIdAtRank(t, "species") (TaxonomyWrapper.cpp:479-498): the first node from t upwards
        whose rank index is not below the species'; a node already above species level (a genus) is
        its own answer. 0 for the root."""
        if t == 1 or t not in self.parent:
            return 0
        x, cnt = t, 0
        while cnt < 30 and _RANK_INDEX.get(self.rank[x], -1) < _RANK_INDEX["species"]:
            x = self.parent[x]
            cnt += 1
        return t if cnt == 30 else x
