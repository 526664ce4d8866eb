"""CPU: the positions `bench.py --dump-outputs` writes of a large value vector are fixed by the vector's length alone (so two
builds of the project can be compared output for output), distinct, sorted, inside the vector and within the dump's 64 MB."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_positions_are_a_fixed_sample_within_the_cap():
    b = _bench()
    cap = b.DUMP_MAX_ENTRIES
    assert b.dump_positions(cap, cap) is None  # written whole
    n = 275462200  # the headline's Jacobian: 256 states x 2000 knots
    pos = b.dump_positions(n, cap)
    assert np.array_equal(pos, _bench().dump_positions(n, cap))
    assert 0.9 * cap < pos.size <= cap and 8 * pos.size < 64 << 20
    assert pos[0] >= 0 and pos[-1] < n and np.all(np.diff(pos) > 0)
