"""mtb_merge_db / mtb_merge_db_dirs: the checks that run on the host before any device call (this
file needs no GPU: on a machine without one a device call would fail with MTB_ERR_HIP instead)."""
import ctypes
import os

import numpy as np

from metabuli_work_amd import synth
from metabuli_work_amd._abi import default_params
from metabuli_work_amd._lib import lib
from metabuli_work_amd.dbbuild import HostDb, MtbDbBuilt, MtbMergeInput, _lib_build, subset_genomes

MTB_ERR_ARG, MTB_ERR_IO = -1, -2


def _call(ins, n_in, split_num=64):
    taxo = synth.make_taxonomy(4, 2, seed=1)
    hdb = HostDb(taxo)
    tax = hdb.c_struct()
    par = default_params(kmer_format=2)
    ids = np.array([int(taxo.taxid[-1])], np.int32)
    out = MtbDbBuilt()
    L = _lib_build()
    rc = L.mtb_merge_db(ins, n_in, ids.ctypes.data, len(ids), ctypes.byref(tax), ctypes.byref(par), split_num, 0,
                        ctypes.byref(out))
    assert lib().mtb_last_error().decode() != ""
    return rc


def test_merge_input_mirror_has_the_headers_size():
    assert ctypes.sizeof(MtbMergeInput) == 16 + 16
    assert [f for f, _ in MtbMergeInput._fields_] == ["diff_idx", "n_diff_idx", "info", "n_info"]
    assert lib().mtb_merge_tile_items() > 0


def test_merge_db_argument_checks():
    one = (MtbMergeInput * 1)()
    many = (MtbMergeInput * 65)()
    assert _call(one, 0) == MTB_ERR_ARG
    assert _call(many, 65) == MTB_ERR_ARG
    assert _call(None, 1) == MTB_ERR_ARG
    assert _call(one, 1, split_num=1) == MTB_ERR_ARG
    bad = (MtbMergeInput * 1)()
    bad[0].n_diff_idx, bad[0].n_info = 4, 2  # counts without arrays
    assert _call(bad, 1) == MTB_ERR_ARG


def _params(d, fmt=2, syncmer=0):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "db.parameters"), "w") as f:
        f.write(f"DB_name\tx\nReduced_alphabet\t0\nAccession_level\t0\nSkip_redundancy\t1\nSyncmer\t{syncmer}\n"
                f"Kmer_format\t{fmt}\n")
    return os.fsencode(d)


def _merge_dirs(dirs, out):
    arr = (ctypes.c_char_p * len(dirs))(*dirs)
    rc = lib().mtb_merge_db_dirs(arr, len(dirs), os.fsencode(out), 64, 0)
    assert lib().mtb_last_error().decode() != ""
    return rc


def test_merge_dirs_refuses_differing_parameters(tmp_path):
    a = _params(str(tmp_path / "a"))
    assert _merge_dirs([a, _params(str(tmp_path / "b"), fmt=1)], str(tmp_path / "o")) == MTB_ERR_ARG
    assert "Kmer_format" in lib().mtb_last_error().decode()
    assert _merge_dirs([a, _params(str(tmp_path / "c"), syncmer=1)], str(tmp_path / "o")) == MTB_ERR_ARG
    assert "Syncmer" in lib().mtb_last_error().decode()
    assert not (tmp_path / "o").exists()


def test_merge_dirs_missing_info_is_an_io_error(tmp_path):
    dirs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        dirs.append(_params(d))
        np.array([0x8001], np.uint16).tofile(os.path.join(d, "diffIdx"))
        with open(os.path.join(d, "taxID_list"), "w") as f:
            f.write("5\n")
    np.array([5], np.uint32).tofile(os.path.join(str(tmp_path / "a"), "info"))
    assert _merge_dirs(dirs, str(tmp_path / "o")) == MTB_ERR_IO
    assert "info" in lib().mtb_last_error().decode()
    assert _merge_dirs([os.fsencode(str(tmp_path / "none"))], str(tmp_path / "o")) == MTB_ERR_IO


def test_subset_genomes_keeps_the_genomes_and_their_blocks():
    """What build_db(parts=k) and update_db's callers build from: a subset holds its genomes'
    sequences, taxIDs and gene blocks unchanged."""
    taxo = synth.make_taxonomy(6, 3, seed=2)
    gen = synth.make_genomes(taxo, genome_len=3000, seed=2)
    idx = [g for g in range(gen.n) if g % 3 == 1]
    sub = subset_genomes(gen, idx)
    assert sub.n == len(idx) and np.array_equal(sub.taxid, gen.taxid[idx])
    assert np.array_equal(sub.species, gen.species[idx])
    for k, g in enumerate(idx):
        assert np.array_equal(sub.seq[int(sub.off[k]):int(sub.off[k + 1])], gen.seq[int(gen.off[g]):int(gen.off[g + 1])])
        m, ms = gen.blk_genome == g, sub.blk_genome == k
        assert m.sum() > 0
        for name in ("blk_start", "blk_end", "blk_strand"):
            assert np.array_equal(getattr(gen, name)[m], getattr(sub, name)[ms])
