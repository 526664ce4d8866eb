"""CPU: what tests/test_gpu_tdb_persistent.py rests on that needs no device -- the scratch-slot formula of DESIGN 4.22 as restated in
tests/tdb_share_cases.py (figures worked out by hand from the formula), option "tdb_resident" at the boundary of a structure-only
handle, and the option documented where options are listed."""
import os

import pytest

import dto_amd
import tdb_share_cases as S
from helpers import to_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "tdb_resident"


def test_the_slot_formula_gives_the_expected_caps():
    # (160, 3, 1, 10), Hessian, two members: np = 160, p = 8, 36 pairs, Q = 44; 45 columns per member on a stride of 64
    assert S.slot_doubles(160, 3, 1, 10, 2, 2) == 4 * 160 * 128 + 160 * 160 + 44 * 64 * 160 + 32 * 160 * 2 + 45 * 44
    mib = lambda *a: round(8 * S.slot_doubles(*a) / 2.0 ** 20, 2)
    assert [mib(160, 3, 1, 10, 2, g) for g in (2, 3, 4, 5)] == [4.35, 6.42, 8.49, 10.56] and mib(256, 7, 0, 12, 2, 2) == 14.67
    assert S.launch_cap(160, 3, 1, 10, 5, True) == 3 and S.launch_cap(160, 3, 1, 10, 4, False) == 4 and S.launch_cap(160, 3, 1, 10, 9, False) == 8
    assert S.launch_cap(256, 7, 0, 12, 2, True) == 1 and S.launch_cap(256, 7, 0, 12, 8, False) == 8
    assert S.launch_cap(65, 1, 0, 2, 9, True) == 8 and S.launch_cap(65, 1, 0, 2, 9, False) == 8 and S.launch_cap(65, 2, 1, 2, 5, True) == 5
    assert S.launch_cap(72, 1, 1, 2, 2, True) == 2 and S.launch_cap(72, 1, 1, 2, 1, True) == 1


def test_further_carriers_leave_the_family_of_two_unchanged():
    G2, m2 = S.family(16, 2, 2, seed=3)
    G5, m5 = S.family(16, 2, 12, seed=3)
    assert (G2 == G5).all() and len(m5) == 12 and all(a[:2] == b[:2] and (a[2] == b[2]).all() for a, b in zip(m2, m5))
    assert len({(k, w) for k, w, _ in m5}) == 12 and len(S.family(16, 2, 0, seed=3)[1]) == 0


def test_a_handle_without_a_persistent_grid_takes_zero_only():
    """Structure-only (no device): no integrator has a grid, whatever its kernel would be."""
    ev = dto_amd.Evaluator(to_engine(S.lone(65, 1, 0, 2, 2, 3)), device=-1)
    try:
        ev.set_option(OPTION, 0)
        for bad in (1, -1, 1 << 40):
            with pytest.raises(dto_amd.EngineError, match=OPTION + r" takes 0 .*\b0\b"):
                ev.set_option(OPTION, bad)
        ev.set_option(OPTION, 0)   # the handle stays usable
    finally:
        ev.close()


def test_a_ninth_integrator_is_refused_so_no_group_exceeds_one_launch_of_eight():
    """Why tests/test_gpu_tdb_persistent.py has no group of nine (8 + 1 launches): a handle takes eight integrators."""
    dto_amd.Evaluator(to_engine(S.problem(8, 8, m=1, order=0, N=3, derivative=False)), device=-1, shared_generators=True).close()
    for po in (S.problem(8, 8, m=1, order=0, N=3), S.problem(8, 9, m=1, order=0, N=3, derivative=False)):
        with pytest.raises(dto_amd.EngineError, match="at most 8 integrators"):
            dto_amd.Evaluator(to_engine(po), device=-1, shared_generators=True)


def test_the_option_is_documented():
    header = open(os.path.join(ROOT, "include", "dto_engine.h"), encoding="utf-8").read()
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    assert '"%s" (default 0' % OPTION in header and OPTION in dto_amd.Evaluator.set_option.__doc__ and "`%s`" % OPTION in design
