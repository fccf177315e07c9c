"""The environment switches of libdqrm: what the sources read is what INTEGRATION.md documents,
and every switch is read in one place (the switch block of csrc/dqrm_host.hip)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deep_quantized_recommendation_model_dqrm_amd", "csrc")


def getenv_calls():
    """[(file name, variable)] for every getenv("DQRM_...") under csrc/."""
    calls = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            calls += [(os.path.basename(path), name) for name in re.findall(r'getenv\(\s*"(DQRM_[A-Z0-9_]+)"', f.read())]
    return calls


def documented():
    """The names in the first column of INTEGRATION.md's table of libdqrm's switches."""
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    m = re.search(r"^#+ Environment switches of libdqrm\n(.*?)(?=^#+ |\Z)", text, flags=re.S | re.M)
    assert m, "INTEGRATION.md has no 'Environment switches of libdqrm' section"
    return re.findall(r"^\| `(DQRM_[A-Z0-9_]+)`", m.group(1), flags=re.M)


def test_every_switch_read_is_documented_and_the_reverse():
    names = documented()
    assert len(names) == len(set(names)), "a switch is listed twice"
    assert {n for _, n in getenv_calls()} == set(names)
    assert len(names) == 16


def test_each_switch_is_read_in_one_place():
    calls = getenv_calls()
    assert calls
    where = {}
    for fname, name in calls:
        where.setdefault(name, []).append(fname)
    assert {n: w for n, w in where.items() if w != ["dqrm_host.hip"]} == {}
