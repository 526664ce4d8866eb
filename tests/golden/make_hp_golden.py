"""Writes tests/golden/hp_*.npz: the accuracy-budget fixtures (tests/hp_cases.py) with expected values from the 320-bit
fixed-point reference tests/hp_reference.py.  Minutes of CPU, no GPU, nothing but numpy:

    python tests/golden/make_hp_golden.py [case ...]

The 130-state case takes a minute and a half, the 250- and 330-state cases seven to eleven minutes each on one core; the cases are
independent, so give each a process of its own.
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


if __name__ == "__main__":
    main(sys.argv[1:])
