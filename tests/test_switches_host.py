"""CPU: the run-time switches have one home.  csrc/api.hip is the only library source that reads the environment (so that
ddpm_reload_env() reaches every switch), and DESIGN 4.1 lists exactly the switches that something reads."""

import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ddpm_ood_amd" / "csrc"


def _load_switches_names():
    body = re.search(r"static void load_switches\(\) \{(.*?)\n\}", (CSRC / "api.hip").read_text(), flags=re.S).group(1)
    return set(re.findall(r'"(DDPM_[A-Z0-9_]+)"', body))


def _design_4_1():
    text = (ROOT / "DESIGN.md").read_text()
    return text[text.index("### 4.1 Run-time switches"):text.index("\n## 5.")]


def test_only_api_hip_reads_the_environment():
    readers = [p.name for p in sorted(CSRC.iterdir()) if p.is_file() and p.name != "api.hip" and "getenv" in p.read_text()]
    assert readers == []


def test_every_parsed_switch_has_a_design_row():
    parsed = _load_switches_names()
    assert len(parsed) >= 30, sorted(parsed)  # (the parser of this test still finds them)
    documented = set(re.findall(r"`(DDPM_[A-Z0-9_]+)", _design_4_1()))
    assert sorted(parsed - documented) == []


def test_every_design_row_names_a_switch_that_something_reads():
    sources = [CSRC / "api.hip", ROOT / "tests" / "conftest.py", ROOT / "bench.py"]
    sources += sorted((ROOT / "ddpm_ood_amd").rglob("*.py")) + sorted((ROOT / "tools").rglob("*.py"))
    read = set()
    for p in sources:
        read |= set(re.findall(r"DDPM_[A-Z0-9_]+", p.read_text()))
    documented = set(re.findall(r"`(DDPM_[A-Z0-9_]+)", _design_4_1()))
    assert len(documented) >= 30, sorted(documented)
    assert sorted(documented - read) == []
