"""The TUNING build's A/B switches: every name csrc/ passes to tune_int or tune_double stands in DESIGN.md's table of the switches
that remain (section 4.10.1), and every name in the table is read by the source.  A switch nothing uses is retired with its code,
not left behind; a new one is written down with the test or tool that uses it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")


def _in_source():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".cpp", ".hip", ".h")):
            with open(os.path.join(CSRC, f)) as fh:
                names |= set(re.findall(r'\btune_(?:int|double)\(\s*"([A-Za-z0-9_]+)"', fh.read()))
    return names


def _in_table():
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        text = fh.read()
    section = text.split("#### 4.10.1 The switches that remain", 1)[1].split("\n#", 1)[0]
    rows = [l for l in section.splitlines() if l.startswith("| `")]
    names = [re.match(r"\| `([A-Za-z0-9_]+)` \|", l).group(1) for l in rows]
    assert len(names) == len(set(names)), names
    # every row says what uses the switch: tests or tools of this repository, which name it
    for name, l in zip(names, rows):
        users = re.findall(r"`((?:tests|tools)/[^`]+)`", l.split("|")[3])
        assert users, l
        for u in users:
            with open(os.path.join(ROOT, u)) as fh:
                assert name in fh.read(), (name, u)
    return set(names)


def test_the_table_of_remaining_switches_is_the_source():
    source, table = _in_source(), _in_table()
    print(sorted(source), sorted(table), sep="\n")
    assert len(source) >= 1
    assert source == table, (sorted(source - table), sorted(table - source))
