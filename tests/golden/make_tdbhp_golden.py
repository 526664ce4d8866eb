"""Writes tests/golden/tdbhp_*.npz: the fixtures of the time-dependent accuracy tests (tests/tdbhp_cases.py) -- inputs, expected
values from the 320-bit reference of the discrete map (tests/tdb_hp_reference.py), and beside them the measured error of the
fp64 yardstick (tests/tdb_large_cases.py) with the bars derived from it (`classes`, `yard`, `bars`).  CPU only, nothing but numpy:

    python tests/golden/make_tdbhp_golden.py [case ...]
    python tests/golden/make_tdbhp_golden.py --scan [case ...]  # tdbhp_scan_*.npz: the rollout and both solves (tests/scan_cases.py)

Seconds for the cases up to 36 states, about a minute each for 128 states and for 72 states with its second member; the cases are
independent, so give each a process of its own.  `--scan` also needs g++ (the scan's index plan): 20 s at most (128 states).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for path in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if path not in sys.path:
        sys.path.insert(0, path)

import tdbhp_cases as C  # noqa: E402


def build(name, intervals=None):
    """The fixture's arrays: inputs, their hash, expected vectors, norms, and (with every interval) the yardstick's errors and the
    bars."""
    d = C.inputs(name)
    out = dict(d)
    out["input_hash"] = np.array(C.input_hash(d))
    out.update(C.expected(name, d, intervals))
    if intervals is None:
        classes, yard, bars = C.bars_from(C.yardstick_errors(name, out))
        out.update(classes=classes, yard=yard, bars=bars)
    return out


def main(names):
    for name in names or list(C.CASES):
        t = time.time()
        arrays = build(name)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: {os.path.getsize(path)} bytes, {time.time() - t:.1f} s, ||dt_k G||_2 = {np.round(arrays['norm2'], 3)}")
        for c, y, b in zip(arrays["classes"], arrays["yard"], arrays["bars"]):
            print(f"  {c:20s} yardstick worst {np.nanmax(y):.2e}  bar {b:.2e}")


def build_scan(case):
    """The scan fixture of a case of tests/scan_cases.py: X0, B, the 320-bit rollout and both solves, the yardstick and the bars."""
    import scan_cases as S
    return S.build_fixture(case)


def main_scan(cases):
    import scan_cases as S
    for case in cases or [c for c in S.CASES if c.startswith("tdbhp_")]:
        t = time.time()
        arrays = build_scan(case)
        path = os.path.join(HERE, S.fixture_name(case) + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{case}: {os.path.getsize(path)} bytes, {time.time() - t:.1f} s, rho = {arrays['rho']}, a-priori bound {float(arrays['rho_bound']):.2e}")
        for q, y, b in zip(S.QUANTITIES, arrays["yard"], arrays["bars"]):
            print(f"  {q:4s} sequential fp64 worst {y.max():.2e}  bars {np.array2string(b, precision=2)}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--scan"]:
        main_scan(sys.argv[2:])
    else:
        main(sys.argv[1:])
