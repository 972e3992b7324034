"""GPU reference-DB builder vs the oracle's IndexCreator restatement: byte-identical files.

Beyond the one random world, the hand-made inputs of tests/build_cases.py put k_target_extract (block
edges, both strands, lengths 21..27 / 47 / 48 and 1 or 2 modulo 3, N / IUPAC / lower-case letters, blank
and zero-window blocks), the species-digit pass count (largest taxID 255 .. 2^24 + 1), k_group_heads /
k_group_reduce / lca_node (accession leaves, genomes on species and genus nodes, groups of up to five)
and k_split_ends with the host dedupe (sizeOfSplit 0, 1, 2, cnt == U, several boundaries in one AA part,
a boundary in the last AA part) at their edges, from host and from device-resident sequence, each built
twice. The oracle's files for these inputs are themselves held to plain-Python expectations on the CPU
(tests/test_build_expect.py)."""
import os

import numpy as np
import pytest
import torch  # before the library is loaded, as in test_gtdb_scale.py: the device-resident inputs are tensors

from metabuli_work_amd import synth
from metabuli_work_amd._abi import default_params
from metabuli_work_amd.dbbuild import build_db, build_db_device
from tests import build_cases as bc
from tests import oracle_ctypes as oc
from tests.dbref import decode_diff

pytestmark = pytest.mark.gpu
FMT_IDS = ["f%ds%dm%d" % f for f in bc.FORMATS]


@pytest.mark.parametrize("fmt,syncmer", [(2, 0), (2, 1), (1, 0)])
def test_builder_matches_oracle_writer(tmp_path, fmt, syncmer):
    taxo = synth.make_taxonomy(12, 3, seed=31)
    gen = synth.make_genomes(taxo, genome_len=15000, strain_div=0.01, seed=32)
    par = default_params(kmer_format=fmt, syncmer=syncmer)
    d = str(tmp_path / "oracle_db")
    oc.build_db(d, par, taxo, gen)
    hdb = build_db(gen, taxo, par, device=0)
    for name, arr in (("diffIdx", hdb.diff_idx), ("info", hdb.info), ("split", hdb.split)):
        ref = np.fromfile(os.path.join(d, name), dtype=arr.dtype)
        assert len(ref) == len(arr), name
        assert np.array_equal(ref, arr), name
    ref_ids = np.loadtxt(os.path.join(d, "taxID_list"), dtype=np.int32, ndmin=1)
    assert np.array_equal(np.sort(ref_ids), np.sort(hdb.taxid_list))


def assert_same_files(hdb, ref, what):
    for name, arr in (("diffIdx", hdb.diff_idx), ("info", hdb.info), ("split", hdb.split)):
        assert arr.dtype == ref[name].dtype, (what, name)
        assert len(ref[name]) == len(arr), (what, name, len(ref[name]), len(arr))
        assert ref[name].tobytes() == arr.tobytes(), (what, name)
    assert np.array_equal(np.sort(ref["taxID_list"]), np.sort(hdb.taxid_list)), what


def device_seq(gen):
    seq = torch.from_numpy(np.ascontiguousarray(gen.seq)).cuda()
    off = torch.from_numpy(np.ascontiguousarray(gen.off).view(np.int64)).cuda()
    return seq, off


def check_case(name, fmt, split_num=4096):
    """Host sequence twice (identical bytes), then device-resident sequence, all equal to the oracle."""
    c = bc.get_case(name)
    ref = bc.oracle_db(name, fmt, split_num)
    par = bc.params(fmt)
    a = build_db(c.gen, c.taxo, par, device=0, split_num=split_num)
    assert_same_files(a, ref, "host sequence")
    b = build_db(c.gen, c.taxo, par, device=0, split_num=split_num)
    for x, y in ((a.diff_idx, b.diff_idx), (a.info, b.info), (a.split, b.split), (a.taxid_list, b.taxid_list)):
        assert x.tobytes() == y.tobytes(), "second build differs"
    d = build_db(c.gen, c.taxo, par, device=0, split_num=split_num, device_seq=device_seq(c.gen))
    assert_same_files(d, ref, "device sequence")


@pytest.mark.parametrize("fmt", bc.FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name", bc.ALL_CASES)
def test_case_matches_oracle(name, fmt):
    check_case(name, fmt)


SPLIT_LABELS = ["size0", "size1", "size2", "exact", "two", "three"]


@pytest.mark.parametrize("fmt", bc.FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("label", SPLIT_LABELS)
def test_split_table_build_rule(label, fmt):
    """kSplitByUnique at split_num chosen from the DB's unique count U (the oracle's): sizeOfSplit 0, 1
    and 2, U an exact multiple of split_num - 1, and tables of 2 and 3 entries. Where U has no divisor
    that gives a sizeOfSplit above 2, "exact" repeats size1 (U = U * 1: exact as well)."""
    U = len(bc.oracle_db("split_world", fmt)["info"])
    sn = bc.split_nums(U)
    check_case("split_world", fmt, sn.get(label, sn["size1"]))


@pytest.mark.parametrize("fmt", bc.FORMATS, ids=FMT_IDS)
def test_split_table_long_aa_parts(fmt):
    """Synonymous-codon variants: one AA part spans several sizeOfSplit, so consecutive boundaries fall in
    one run (the host's g == last), and the last boundary lies in the DB's last AA part (g >= U)."""
    values = decode_diff(bc.oracle_db("synonymous", fmt)["diffIdx"])
    check_case("synonymous", fmt, bc.synonymous_split_num(values))


@pytest.mark.parametrize("from_device", [False, True], ids=["host_seq", "device_seq"])
@pytest.mark.parametrize("name", bc.ALL_CASES)
def test_device_out_format1(name, from_device):
    """MTB_BUILD_DEVICE_OUT in format 1, where the values come back as they are (format 2's rank form is
    covered in test_gtdb_scale.py): the decoded oracle diffIdx and its info."""
    fmt = (1, 0, 5)
    c = bc.get_case(name)
    ref = bc.oracle_db(name, fmt)
    v, t = build_db_device(c.gen, c.taxo, bc.params(fmt), device=0,
                           device_seq=device_seq(c.gen) if from_device else None)
    assert np.array_equal(v.cpu().numpy().view(np.uint64), decode_diff(ref["diffIdx"]))
    assert np.array_equal(t.cpu().numpy().view(np.uint32), ref["info"])
