"""The common-k-mer filter's cases (tests/golden/ref_group_filter.npz): the plain-Python diffIdx encoder and
split table the fixture's DB files are written with, the tables of scanner configurations and DBs, the
decoding of the stored fixture, and the filter's predicate in numpy.

The fixture stores per scanner configuration the extracted instances (value, seqID, pos, frame) in
(seqID, frame, pos) order — format 3's in full, the syncmer configurations' as bit masks over format 3's
(a syncmer scanner emits a subset of the plain scanner's windows; the generator asserts it) — and per
DB: which of the configuration's distinct values it holds (a bit mask), how many values of no read are
added (foreign_values regenerates them), the reference's kept instances and hit positions as bit masks
over the instances, and the kept count. db_values() puts a DB's values together again, duplicates
included; write_db() writes them as the files filterCommonKmers reads.
"""
import pathlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "ref_group_filter.npz"

CONFIGS = [("fmt3", 0, 5), ("fmt5_s5", 1, 5), ("fmt5_s6", 1, 6)]  # name, syncmer, smer_len
DBS = ("fifth", "all", "none")  # about a fifth of the instances hit; every value; none of them
SPLITS = (4, 4096)
FOREIGN = 4600          # values of no read in every DB: more k-mers than the larger split table has entries
DUP_EVERY = 7           # every 7th DB value is written twice (one entry per value and species)
AA_PART = ~np.uint64(0xFFFFFF)
SPLIT_DTYPE = np.dtype([("ADkmer", "<u8"), ("diffIdxOffset", "<u8"), ("infoIdxOffset", "<u8")])


# ---- diffIdx and split --------------------------------------------------------------
def encode_diffidx(values) -> np.ndarray:
    """Ascending values as diffIdx words: per value its delta from the one before (the first from 0) in
    15-bit groups, most significant first, bit 15 set on the last group only."""
    words, last = [], 0
    for v in (int(x) for x in values):
        d = v - last
        assert d >= 0, "values descend"
        groups = [d & 0x7FFF]
        d >>= 15
        while d:
            groups.append(d & 0x7FFF)
            d >>= 15
        groups.reverse()
        groups[-1] |= 0x8000
        words += groups
        last = v
    return np.array(words, np.uint16)


def decode_diffidx(words) -> np.ndarray:
    out, acc, last = [], 0, 0
    for w in (int(x) for x in words):
        acc = (acc << 15) | (w & 0x7FFF)
        if w & 0x8000:
            last += acc
            out.append(last)
            acc = 0
    assert acc == 0, "ends mid k-mer"
    return np.array(out, np.uint64)


def split_table(values, n_entries: int) -> np.ndarray:
    """Entry 0 is zero; entry i >= 1 is the first k-mer of a new AA group (the bits above the low 24) after
    the i-th multiple of len(values) // (n_entries - 1) k-mers: its value, the diffIdx words and the k-mers
    written so far, that k-mer included. Unused trailing entries stay zero."""
    split = np.zeros(n_entries, SPLIT_DTYPE)
    size = len(values) // (n_entries - 1)
    nxt, boundary, pending, aa_at = 1, 1, False, None
    words = 0
    last = 0
    for j, v in enumerate(int(x) for x in values):
        d = v - last
        words += max(1, (d.bit_length() + 14) // 15)
        last = v
        aa = v & ~0xFFFFFF
        if pending and aa != aa_at and nxt < n_entries:
            split[nxt] = (v, words, j + 1)
            nxt += 1
            pending = False
        if boundary < n_entries and j + 1 == boundary * size:
            aa_at, pending = aa, True
            boundary += 1
    return split


def write_db(db_dir, values, n_entries: int = 4, params=None) -> None:
    """diffIdx and split of a common-k-mer DB (and kmer_params from a dict of its three keys)."""
    d = pathlib.Path(db_dir)
    d.mkdir(parents=True, exist_ok=True)
    encode_diffidx(values).tofile(d / "diffIdx")
    split_table(values, n_entries).tofile(d / "split")
    if params is not None:
        (d / "kmer_params").write_text("".join(f"{k} {v}\n" for k, v in params.items()))


# ---- the stored fixture ---------------------------------------------------------------------------------
def load():
    return np.load(GOLDEN)


def _bits(fx, key, n):
    return np.unpackbits(fx[key])[:n].astype(bool)


def extraction(fx, cfg: str):
    """(value, seqID, pos, frame) of a configuration's instances, in (seqID, frame, pos) order."""
    v, s, p, f = fx["fmt3_value"], fx["fmt3_seq"], fx["fmt3_pos"], fx["fmt3_frame"]
    if cfg == "fmt3":
        return v, s, p, f
    m = _bits(fx, f"{cfg}_mask", len(v))
    return v[m], s[m], p[m], f[m]


def foreign_values(n: int, exclude) -> np.ndarray:
    """n distinct 60-bit values that are none of `exclude`, the same on every call."""
    rng = np.random.default_rng(20261021)
    out = np.unique(rng.integers(1, 1 << 60, 2 * n + 64, dtype=np.uint64))
    out = out[~np.isin(out, exclude)]
    rng.shuffle(out)
    return np.sort(out[:n])


def db_values(fx, cfg: str, db: str) -> np.ndarray:
    """A DB's values as written to its diffIdx: ascending, every DUP_EVERY-th twice."""
    distinct = np.unique(extraction(fx, cfg)[0])
    own = distinct[_bits(fx, f"{cfg}_{db}_own", len(distinct))]
    vals = np.sort(np.concatenate([own, foreign_values(FOREIGN, distinct)]))
    return np.repeat(vals, 1 + (np.arange(len(vals)) % DUP_EVERY == 0))


def reference_result(fx, cfg: str, db: str):
    """(keep mask over the instances, hit (seqID, pos) pairs sorted, kept count) as the reference gave them."""
    v, s, p, _ = extraction(fx, cfg)
    keep = _bits(fx, f"{cfg}_{db}_keep", len(v))
    at_hit = _bits(fx, f"{cfg}_{db}_hitpos", len(v))
    pairs = np.unique(np.stack([s[at_hit], p[at_hit]], 1), axis=0) if at_hit.any() else np.zeros((0, 2), np.uint32)
    return keep, pairs, int(fx[f"{cfg}_{db}_kept"])


# ---- the predicate --------------------------------------------------------------------------------------
def predicate(db, value, seq, pos):
    """(hit, keep): an instance is hit iff its value is in db; it is kept iff no hit instance of its read
    lies within one nucleotide of it (itself included)."""
    value, db = np.asarray(value, np.uint64), np.asarray(db, np.uint64)
    hit = np.isin(value, db)
    key = np.asarray(seq, np.int64) * (1 << 33) + np.asarray(pos, np.int64) + 1  # pos - 1 stays inside the read's keys
    hk = np.unique(key[hit])
    removed = np.isin(key - 1, hk) | np.isin(key, hk) | np.isin(key + 1, hk)
    return hit, ~removed


def multiset(*cols):
    """Rows sorted, for comparing multisets of (value, seqID, pos) tuples."""
    a = np.stack([np.asarray(c, np.uint64) for c in cols], 1)
    return a[np.lexsort(a.T[::-1])]
