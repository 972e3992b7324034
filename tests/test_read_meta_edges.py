"""K0 (k_read_meta) reduces the batch's two maxima per block: a block takes 4 stretches of 256 reads,
each wave reduces its lanes, the waves meet in LDS, and one thread issues at most two atomicMax. The
maxima choose the uniform-unit layout (maxW[0]: the most windows in one frame of one read) and K1F's
form (maxW[1]: the longest mate past kSeqMate = 219 bases, 0 when there is none), so a value lost at a
wave, stretch or block edge shows as a wrong layout, a stage overflow, or results that differ from the
oracle's.

Batches of 1, 255, 256, 257 and 513 pairs (one block, with 1, 2 and 3 stretches in part), and of 1023,
1024, 1025 and 2049 (the first block's last read, a second and third block of one read):
  * the only pair with a window sits at a stretch's first or last thread, at a block's, or last in the
    batch; every other pair has two 12-base mates;
  * every pair is empty: both maxima 0, nothing classifies;
  * the only mate past 219 bases sits beside a mate without a window (the pair adds nothing to maxW[0]: the
    batch stays uniform, and only maxW[1] keeps it out of K1F's LDS stage) at read 0, 255 / 256, a block's
    edge, and last.
Each batch is compared with the oracle as tests/test_batch_shapes.py compares: query k-mers with info,
matches, results, taxID:count lists, the units the batch took."""
import numpy as np
import pytest

from metabuli_work_amd import synth
from tests import oracle_ctypes as oc
from tests.test_batch_shapes import Case, _compare, _genome_pair, _oracle_stages, _reads, check_oracle_alone, covered

SIZES = [1, 255, 256, 257, 513, 1023, 1024, 1025, 2049]
N_SAMPLED = 64  # distinct 150/150 pairs; a batch repeats them


def positions(n):
    """Read indices at the edges: of a 64-lane wave, a 256-read stretch, a 1024-read block, the batch."""
    return sorted({p for p in (0, 63, 64, 255, 256, 1023, 1024, 2047, 2048, n - 1) if p < n})


def build_cases(gen, n):
    base = synth.make_reads(gen, N_SAMPLED, seed=23)
    b1 = [np.asarray(base.seq1[int(base.off1[i]):int(base.off1[i + 1])]) for i in range(N_SAMPLED)]
    b2 = [np.asarray(base.seq2[int(base.off2[i]):int(base.off2[i + 1])]) for i in range(N_SAMPLED)]
    assert all(len(a) == 150 and len(b) == 150 for a, b in zip(b1, b2))
    e1, e2 = _genome_pair(gen, 1, 12, 12)
    whole = _genome_pair(gen, 4, 150, 150)  # a pair without substitutions: it has matches
    cases = []
    for p in positions(n):
        m1, m2 = [e1] * n, [e2] * n
        m1[p], m2[p] = whole
        cases.append(Case(f"window_at_{p}", _reads(m1, m2), empty={i: covered(12) * 2 for i in {0, n - 1} - {p}},
                          uniform=12, matched=(p,)))
    cases.append(Case("all_empty", _reads([e1] * n, [e2] * n), empty={i: covered(12) * 2 for i in (0, n - 1)},
                      uniform=12, nothing=True))
    for j, p in enumerate(positions(n)):
        m1 = [b1[i % N_SAMPLED] for i in range(n)]
        m2 = [b2[i % N_SAMPLED] for i in range(n)]
        l1, l2 = ((5000, 15), (25, 220))[j % 2]  # far past the stage, and one base past kSeqMate
        m1[p], m2[p] = _genome_pair(gen, p, l1, l2)
        cases.append(Case(f"long_at_{p}", _reads(m1, m2), empty={p: covered(l1) + covered(l2)}, uniform=12))
    return cases


@pytest.fixture(scope="module")
def fmt2(make_db):
    db_dir, taxo, gen = make_db("fmt2")
    odb = oc.OracleDb(db_dir)
    yield db_dir, gen, odb
    odb.close()


def test_positions_cover_the_edges():
    assert positions(1) == [0]
    assert positions(257) == [0, 63, 64, 255, 256]
    assert positions(1025) == [0, 63, 64, 255, 256, 1023, 1024]
    assert positions(2049)[-3:] == [1024, 2047, 2048]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_read_meta_block_reduction(fmt2, n):
    from metabuli_work_amd.classifier import Classifier
    from metabuli_work_amd._lib import MtbError
    from tests.test_gpu_parity import _params
    db_dir, gen, odb = fmt2
    par = _params(db_dir, 2)
    failures = []
    with Classifier(par, db_dir=db_dir) as clf:
        for case in build_cases(gen, n):
            o = _oracle_stages(odb, par, case.reads)
            check_oracle_alone(case, o[2], o[1])
            if case.name.startswith("long_at_") and n > 1:
                assert int(o[2]["is_classified"].sum()) >= (n - 1) // 2, case.name
            r = case.reads
            try:
                br = clf.classify_batch(r.seq1, r.off1, r.seq2, r.off2, keep_stages=True)
            except MtbError as e:  # a mate past kSeqMate in the LDS stage is refused by K1F's guard
                failures.append(f"{case.name}: {e}")
                continue
            failures += [f"{case.name}: {b}" for b in _compare(clf, case, br, par, db_dir, o, {})]
    assert not failures, "\n".join(failures)
