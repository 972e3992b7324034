"""numpy restatements of the common-k-mer DB build (create_common_kmer_list: extractKmer_dna2aa over
six frames, mergeTargetFiles<COMMON_KMER>) that tests/test_gpu_common.py takes its expected values from
(never from the code under test). tests/test_ref_common.py holds them byte for byte to the reference's
own output (tests/golden/ref_common.npz).

The definition built to: for every distinct AA 12-mer value over all genomes, S = the species of the
genomes that hold it; the DB holds the value iff |S| >= 2, info = LCA(S); values ascending, each once;
the split table by the merge's rule with the whole value as AminoAcidPart (kmer_format 3 / 5), its
sizeOfSplit from the number of k-mers before the merge."""
import numpy as np

from tests import pyscan
from tests.dbref import diff_words
from tests.group_filter_cases import encode_diffidx

K = 12

# byte -> 2-bit code as pyscan reads it (7: not a base), and the 5 x 5 x 5 translation table
_CODE = np.array([pyscan.code(pyscan.ATCG[b]) for b in range(256)], np.int64)
_RC_CODE = np.array([pyscan.code(pyscan.IRCT[pyscan.ATCG[b]]) for b in range(256)], np.int64)
_AA = np.full((8, 8, 8), -1, np.int64)
for (_a, _b, _c), _v in pyscan.AA.items():
    _AA[_a, _b, _c] = _v


def frame_bounds(n: int, frame: int):
    """extractKmer_dna2aa (KmerExtractor.cpp:401-411): (begin, end) of a frame, end inclusive."""
    return (frame, n - 1) if frame < 3 else (0, n - 1 - frame % 3)


def frame_aa(seq: bytes, frame: int) -> np.ndarray:
    """The frame's codons translated in scan order (-1: does not translate): from `begin` rightwards on a
    forward frame, from `end` leftwards on the reverse complement (KmerScanner.h:231-237)."""
    s = np.frombuffer(seq, np.uint8)
    begin, end = frame_bounds(len(s), frame)
    n = max(0, (end - begin + 1) // 3)
    if n == 0:
        return np.zeros(0, np.int64)
    j = np.arange(n)
    if frame < 3:
        lo = begin + 3 * j
        return _AA[_CODE[s[lo]], _CODE[s[lo + 1]], _CODE[s[lo + 2]]]
    ci = end - 3 * j
    return _AA[_RC_CODE[s[ci]], _RC_CODE[s[ci - 1]], _RC_CODE[s[ci - 2]]]


def frame_kmers(seq: bytes, frame: int, syncmer: int = 0, smer: int = 5) -> np.ndarray:
    """The values KmerScanner_dna2aa(12) / SyncmerScanner_dna2aa(12, smer) emit over one frame, in scan
    order: every window of 12 translating codons; with syncmers those whose earliest minimal s-mer is the
    first or the last."""
    aa = frame_aa(seq, frame)
    w = len(aa) - K + 1
    if w <= 0:
        return np.zeros(0, np.uint64)
    bad = np.concatenate([[0], np.cumsum(aa < 0)])
    ok = (bad[K:] - bad[:-K]) == 0
    a = np.where(aa < 0, 0, aa).astype(np.uint64)
    val = np.zeros(w, np.uint64)
    for k in range(K):
        val = (val << np.uint64(5)) | a[k:k + w]
    if syncmer:
        n_sm = K - smer + 1
        sm = np.zeros(len(aa) - smer + 1, np.uint64)
        for k in range(smer):
            sm = (sm << np.uint64(5)) | a[k:k + len(sm)]
        best = np.argmin(np.stack([sm[q:q + w] for q in range(n_sm)]), axis=0)  # the first minimum
        ok &= (best == 0) | (best == n_sm - 1)
    return val[ok]


def genome_kmers(seq: bytes, syncmer: int = 0, smer: int = 5) -> np.ndarray:
    """extractKmer_dna2aa: the six frames' values, frame after frame."""
    return np.concatenate([frame_kmers(seq, f, syncmer, smer) for f in range(6)])


def species_pairs(per_genome_values, species):
    """The distinct (value, species) pairs of genomes with the given species, in (value, species) order."""
    if not len(per_genome_values):
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    v = np.concatenate([np.asarray(x, np.uint64) for x in per_genome_values])
    s = np.concatenate([np.full(len(x), sp, np.int64) for x, sp in zip(per_genome_values, species)])
    if len(v) == 0:
        return v, s
    o = np.lexsort((s, v))
    v, s = v[o], s[o]
    head = np.ones(len(v), bool)
    head[1:] = (v[1:] != v[:-1]) | (s[1:] != s[:-1])
    return v[head], s[head]


def common_rule(tree, v, s):
    """mergeTargetFiles<COMMON_KMER> over distinct (value, species) pairs in (value, species) order:
    (values held by two or more species, the LCA of each one's species)."""
    if len(v) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    starts = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
    ends = np.concatenate([starts[1:], [len(v)]])
    keep_v, keep_i = [], []
    for a, b in zip(starts.tolist(), ends.tolist()):
        if b - a < 2:
            continue
        red = int(s[a])
        for x in s[a + 1:b].tolist():
            red = tree.lca(red, int(x))
        keep_v.append(v[a])
        keep_i.append(red)
    return np.array(keep_v, np.uint64), np.array(keep_i, np.uint32)


def common_split(values, n_before: int, split_num: int) -> np.ndarray:
    """IndexCreator.h:432-447 with kmer_format 3's AminoAcidPart (the whole value): sizeOfSplit =
    numOfKmerBeforeMerge / (splitNum - 1); after every sizeOfSplit written k-mers the next k-mer of another
    value opens an entry (its value, the diffIdx words and k-mers written so far, itself included)."""
    size = n_before // (split_num - 1)
    offsets = [k * size for k in range(split_num)] + [None]
    split = np.zeros(3 * split_num, np.uint64)
    words = diff_words(values)
    offset_idx, split_idx, check, aa_tmp, diff_cnt = 1, 1, 0, None, 0
    for i in range(len(values)):
        diff_cnt += int(words[i])
        if check == 1 and int(values[i]) != aa_tmp:
            split[3 * split_idx:3 * split_idx + 3] = (values[i], diff_cnt, i + 1)
            split_idx += 1
            check = 0
        if i + 1 == offsets[offset_idx]:
            aa_tmp = int(values[i])
            check = 1
            offset_idx += 1
    return split


def expected_from_pairs(tree, v, s, n_before: int, split_num: int):
    """(diffIdx, info, split, values) of the DB over the distinct pairs (v, s)."""
    values, info = common_rule(tree, v, s)
    return encode_diffidx(values), info, common_split(values, n_before, split_num), values


def expected_db(tree, seqs, taxids, syncmer: int, smer: int, split_num: int):
    """The DB of genomes `seqs` (bytes) with taxIDs `taxids`: (diffIdx, info, split, taxID list, values).
    The k-mers before the merge are the distinct (value, species) pairs over all genomes."""
    species = [int(tree.sp[t]) for t in taxids]
    v, s = species_pairs([genome_kmers(q, syncmer, smer) for q in seqs], species)
    diff, info, split, values = expected_from_pairs(tree, v, s, len(v), split_num)
    return diff, info, split, np.unique(np.asarray(taxids, np.int32)), values
