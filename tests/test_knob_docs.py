"""INTEGRATION.md's "Environment knobs" section lists exactly the MTB_* variables the library reads:
every name csrc/ passes to getenv is documented there, and every name documented there is read by
csrc/, defined by include/mtb_gpu.h, or one of the benchmark's own MTB_BENCH_* variables."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parents[1]
NAME = re.compile(r"MTB_[A-Z0-9_]*[A-Z0-9]")


def _read_knobs():
    names = set()
    for f in sorted((ROOT / "metabuli_work_amd" / "csrc").iterdir()):
        if f.suffix in (".hip", ".cpp", ".h"):
            names |= set(re.findall(r'getenv\(\s*"(MTB_[A-Z0-9_]+)"', f.read_text()))
    return names


def _documented_knobs():
    text = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"^## Environment knobs\n(.*?)(?=^## )", text, re.M | re.S)
    assert m, 'INTEGRATION.md has no "## Environment knobs" section'
    return set(NAME.findall(m.group(1)))


def test_every_knob_read_is_documented():
    read = _read_knobs()
    assert len(read) > 40  # the scan found the library's getenv calls
    missing = sorted(read - _documented_knobs())
    assert not missing, f"read by csrc/ but not in INTEGRATION.md's Environment knobs: {missing}"


def test_every_documented_knob_exists():
    header = set(NAME.findall((ROOT / "include" / "mtb_gpu.h").read_text()))
    stale = sorted(n for n in _documented_knobs() - _read_knobs() - header if not n.startswith("MTB_BENCH_"))
    assert not stale, f"in INTEGRATION.md's Environment knobs but read by nothing: {stale}"
