"""Writes tests/golden/hp_*.npz: the accuracy-budget fixtures (tests/hp_cases.py) with expected values from the 320-bit
fixed-point reference tests/hp_reference.py.  Minutes of CPU, no GPU, nothing but numpy:

    python tests/golden/make_hp_golden.py [case ...]
    python tests/golden/make_hp_golden.py --scan [case ...]     # hp_scan_*.npz: the rollout and both solves (tests/scan_cases.py)

The 130-state case takes a minute and a half, the 250- and 330-state cases seven to eleven minutes each on one core; the cases are
independent, so give each a process of its own.  `--scan` also needs SciPy (the fp64 yardstick) and g++ (the scan's index plan): seconds
up to 66 states, half a minute at 130, a minute and a half at 250 and two at 330 states.
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

import hp_cases as C  # noqa: E402


def build(name):
    """The fixture's arrays: inputs, their hash, expected vectors, norms."""
    d = C.inputs(name)
    out = dict(d)
    out["input_hash"] = np.array(C.input_hash(d))
    out.update(C.expected(name, d))
    return out


def main(names):
    for name in names or list(C.CASES):
        t = time.time()
        arrays = build(name)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: {os.path.getsize(path)} bytes, {time.time() - t:.1f} s, ||A_k||_2 = {np.round(arrays['norm2'], 3)}, "
              f"||A_k||_1 = {np.round(arrays['norm1'], 2)}")


def build_scan(case):
    """The scan fixture of a case of tests/scan_cases.py: X0, B, the 320-bit rollout and both solves, the yardstick and the bars."""
    import scan_cases as S
    return S.build_fixture(case)


def main_scan(cases):
    import scan_cases as S
    for case in cases or [c for c in S.CASES if c.startswith("hp_")]:
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
