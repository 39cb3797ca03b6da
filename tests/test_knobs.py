"""Environment switches: csrc/knobs.h is the only engine source that reads the environment, and INTEGRATION.md §4's
environment table lists exactly the switches it reads (plus NGP_ENGINE_LIB, read by _capi.py). Text only: no engine
library needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "instant-ngp_amd")
CSRC = os.path.join(PKG, "csrc")
NAME = re.compile(r"NGP_[A-Z0-9_]+")


def read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def env_names_read(path):
    """the NGP_* names a source passes as string literals (what it can look up in the environment)"""
    return set(re.findall(r'"(NGP_[A-Z0-9_]+)"', read(path)))


def env_table_rows():
    """first cells of the rows of §4's environment table (the table whose header starts with `Variable`)"""
    text = read(os.path.join(ROOT, "INTEGRATION.md"))
    sec = text[text.index("\n## 4."):]
    nxt = sec.find("\n## ", 1)
    lines = (sec if nxt < 0 else sec[:nxt]).split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("| Variable |"))
    rows = []
    for l in lines[start + 2:]:
        if not l.startswith("|"):
            break
        rows.append(l.split("|")[1].strip())
    return rows


def test_knobs_header_is_the_only_reader_and_the_table_matches():
    for name in sorted(os.listdir(CSRC)):
        if name != "knobs.h" and os.path.isfile(os.path.join(CSRC, name)):
            assert "getenv" not in read(os.path.join(CSRC, name)), f"csrc/{name} reads the environment: move it to knobs.h"
    knobs = env_names_read(os.path.join(CSRC, "knobs.h"))
    assert len(knobs) >= 27, sorted(knobs)
    rows = [r for r in env_table_rows() if not r.startswith("`-D")]  # build flags are no environment switches
    listed = [n for r in rows for n in NAME.findall(r)]
    for n in sorted(knobs):
        assert listed.count(n) == 1, f"{n} (knobs.h) is in {listed.count(n)} rows of INTEGRATION.md §4's environment table"
    other = env_names_read(os.path.join(PKG, "_capi.py"))
    for n in listed:
        assert n in knobs or n in other, f"INTEGRATION.md §4 lists {n}, which neither knobs.h nor _capi.py reads"
