"""The environment knobs the library reads and the ones INTEGRATION.md section 6
documents are the same set, and only csrc/api.hip reads the environment.
Source text is read for knob names only."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "koordinator_amd" / "csrc"

# std::getenv("KOORDHIP_X"), and read_place_knobs' two wrappers of it: on("KOORDHIP_X"), num("KOORDHIP_X", unset)
READ = re.compile(r'\b(?:getenv|on|num)\(\s*"(KOORDHIP_[A-Z0-9_]+)"')
LITERAL = re.compile(r'"(KOORDHIP_[A-Z0-9_]+)"')
NAME = re.compile(r"KOORDHIP_[A-Z0-9_]+")

# documented in the table, read elsewhere: abi.py loads the library it names; batch_pods is a config field
NOT_IN_CSRC = {"KOORDHIP_LIB"}
NOT_ENV_ROWS = {"koordhip_config.batch_pods"}


def _sources():
    return sorted(p for p in CSRC.iterdir() if p.is_file() and p.name != "Makefile")


def _read_names():
    names = set()
    for p in _sources():
        names |= set(READ.findall(p.read_text()))
    return names


def _documented_names():
    text = (ROOT / "INTEGRATION.md").read_text()
    sec = text[text.index("## 6. Tuning knobs"):]
    nxt = sec.find("\n## ", 1)
    sec = sec if nxt < 0 else sec[:nxt]
    names, other = set(), set()
    for line in sec.splitlines():
        if not line.startswith("|") or line.startswith("|---") or line.startswith("| knob"):
            continue
        first = line.split("|")[1]
        found = NAME.findall(first)
        names |= set(found)
        if not found:
            other.add(first.strip().strip("`"))
    return names, other


def test_getenv_only_in_api_hip():
    readers = [p.name for p in _sources() if "getenv" in p.read_text()]
    assert readers == ["api.hip"], readers


def test_every_knob_literal_is_a_read():
    # no third wrapper hides a name from READ: every exact "KOORDHIP_X" string literal in csrc is an environment read
    literals = set()
    for p in _sources():
        literals |= set(LITERAL.findall(p.read_text()))
    assert literals == _read_names(), sorted(literals ^ _read_names())


def test_documented_knobs_equal_read_knobs():
    read = _read_names()
    documented, other = _documented_names()
    assert len(read) > 20 and other == NOT_ENV_ROWS, (len(read), other)
    assert documented - NOT_IN_CSRC == read, sorted((documented - NOT_IN_CSRC) ^ read)
    assert NOT_IN_CSRC <= documented
    assert "KOORDHIP_LIB" in (ROOT / "koordinator_amd" / "abi.py").read_text()
