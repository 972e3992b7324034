"""The tests' Python restatement of the read grouping (tests/group_expect.py) against what the
reference's own code computed (tests/golden/ref_groups.npz, group_defaults.json: made by
tests/golden/make_ref_groups.py), and the fixture against the designed cases. No GPU."""
import functools
import json
import pathlib

import numpy as np
import pytest

from tests import group_cases, group_expect

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


@functools.lru_cache(maxsize=None)
def ref():
    return np.load(GOLDEN / "ref_groups.npz")


@functools.lru_cache(maxsize=None)
def cases():
    return group_cases.cases()


CASE_NAMES = [c[0] for c in group_cases.cases()]


def test_fixture_holds_every_designed_case():
    g = ref()
    assert list(g["names"]) == CASE_NAMES
    assert bool(g["threads_agree"]) and list(g["threads"]) == [1, 3, 16] and bool(g["sanitizer_clean"])
    for name, n, edges, core, weak in cases():
        assert np.array_equal(g[f"{name}_edges"], edges), name
        assert list(g[f"{name}_shape"]) == [n, core, weak], name
        assert g[f"{name}_maps"].shape == (3, n + 1)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_python_phases_equal_reference(name):
    _, n, edges, core, weak = next(c for c in cases() if c[0] == name)
    got = group_expect.phases(n, edges, core, weak)
    want = ref()[f"{name}_maps"]
    for p in range(3):
        assert np.array_equal(got[p], want[p]), f"{name}: groupMap after phase {('1', '1.5', '2')[p]}"


def test_designed_cases_show_what_they_were_designed_for():
    m = {name: ref()[f"{name}_maps"] for name in CASE_NAMES}
    assert (m["chain_shuffled_ids"][0][1:5001] == 1).all() and not m["chain_shuffled_ids"][2][5001:].any()
    assert (m["star_centre_largest"][0][[1, 3, 95, 96]] == 1).all() and m["star_centre_largest"][2][2] == 0
    assert m["bridge_at_core"][2][10] == 10 and m["bridge_above_core"][0][10] == 1
    wb = m["weak_boundary"][2]
    assert (wb[20], wb[22], wb[23], wb[24], wb[26]) == (0, 22, 22, 24, 26) and m["weak_boundary"][1][24] == 0
    s = m["support_one_and_two"]
    assert s[0][3] == 3 and s[1][3] == 1 and s[1][5] == 5 and s[2][5] == 5
    j = m["singleton_joins_group"]
    assert j[0][7] == 0 and j[1][7] == 1 and j[2][20] == 20 and j[2][21] == 20
    w = m["weak_singletons"]
    assert w[1][8] == 0 and w[2][8] == 8 and w[2][30] == 8 and w[2][31] == 0
    assert m["merge_lowers_label"][0][5] == 5 and m["merge_lowers_label"][1][5] == 2
    assert m["merge_two_groups_lowers_label"][0][40] == 40 and m["merge_two_groups_lowers_label"][1][41] == 3
    # 65535 > core 65534 joins 1 and 2; 65534 is one weak link from read 3 (no support of 2, and Phase 2
    # may not use the grouped read 2); 65533 is not above the weak threshold
    assert list(m["weight_65535"][0][1:6]) == [1, 1, 0, 0, 0] and list(m["weight_65535"][2][1:6]) == [1, 1, 0, 0, 0]
    assert list(m["weight_65535_default_thr"][2][1:5]) == [1, 1, 0, 0]
    assert not m["no_edges"].any() and not m["one_read"].any()
    assert (m["support_chain"][1][[10, 11, 20, 21, 30, 31]] == 10).all()


def test_cap_from_quantile_and_buckets_equal_reference():
    g = ref()
    assert len(g["cap_value"]) == len(g["cap_quantile"]) > 50
    for q, h, want in zip(g["cap_quantile"], g["cap_hist"], g["cap_value"]):
        assert group_expect.cap_from_quantile(h.tolist(), q) == int(want), (q, h[:12])
    assert len(set(g["cap_value"].tolist())) > 4
    for m, want in zip(g["bucket_m"].tolist(), g["bucket_value"].tolist()):
        assert group_expect.m_hist_bucket(m) == want, m


def test_thresholds_restated():
    # the operating points the reference's comments quote: 49.6 k-mers per read -> 15, band (5, 15]
    assert group_expect.thresholds(0.3, 0.3333, 496, 10) == (15, 5)
    assert group_expect.thresholds(0.3, 0.3333, 34 * 3, 1)[0] == 31
    assert group_expect.thresholds(1.0, 0.9999, 2, 1) == (2, 1)  # the clamp to coreThr - 1
    assert group_expect.thresholds(1.0, 1e-6, 40, 1) == (40, 1)  # the clamp to 1
    with pytest.raises(ValueError):
        group_expect.thresholds(0.3, 0.3333, 4, 1)
    for _, n, _, core, weak in cases():
        ratio, band, total = group_cases.params_for(core, weak, n)
        assert group_expect.thresholds(ratio, band, total, n) == (core, weak)


def test_defaults_equal_reference_text():
    """GroupParams' defaults are setGroupGenerationDefaults' (group_defaults.json), field by field; the
    rest of that function's assignments have no place in the grouping parameters."""
    import dataclasses

    from metabuli_work_amd.grouping import GroupParams

    d = json.loads((GOLDEN / "group_defaults.json").read_text())["defaults"]
    fields = {"maxKmerReads": "max_kmer_reads", "maxKmerQuantile": "max_kmer_quantile",
              "minOverlapRatio": "min_overlap_ratio", "weakBandRatio": "weak_band_ratio",
              "mergeSupportRatio": "merge_support_ratio", "mergeMaxUnitReads": "merge_max_unit_reads",
              "syncmer": "syncmer", "smerLen": "smer_len", "seqMode": "seq_mode"}
    outside = {"maxTmpDiskMiB", "verbosity", "ramUsage", "printLog", "maskMode", "maskProb", "matchPerKmer"}
    assert set(d) == set(fields) | outside
    p = GroupParams()
    assert {f.name for f in dataclasses.fields(p)} == set(fields.values())
    for ref_name, ours in fields.items():
        assert getattr(p, ours) == d[ref_name]["value"], ref_name
    assert d["maskMode"]["value"] == 0  # masking is out of scope


def test_library_defaults_equal_reference_text():
    from metabuli_work_amd.grouping import GroupParams

    lib_defaults, py = GroupParams.defaults(), GroupParams()
    assert np.float32(lib_defaults.min_overlap_ratio) == np.float32(py.min_overlap_ratio)
    assert np.float32(lib_defaults.weak_band_ratio) == np.float32(py.weak_band_ratio)
    for f in ("seq_mode", "syncmer", "smer_len", "max_kmer_reads", "max_kmer_quantile", "merge_support_ratio",
              "merge_max_unit_reads"):
        assert getattr(lib_defaults, f) == getattr(py, f), f
