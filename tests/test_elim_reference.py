"""CPU: the NumPy restatement of the whole-dynamics block elimination (elim_cases.eliminate) against numpy.linalg.solve on the block MM
assembled from the oracle's Jacobian, in both directions -- and the same comparison with the algorithm broken in one way at a time,
which must miss the bar by orders of magnitude.

Bar.  Both sides solve the same matrix backward-stably (the elimination multiplies by orthogonal or near-orthogonal propagators and
adds), so each differs from the exact solution by a modest multiple of cond(MM) eps relative to the solution's norm; the bar is
64 cond_2(MM) eps on max |difference| / max |solution|, with cond_2 computed for the case (15 .. 85 on the skew cases).  The
largest difference seen is 6e-15."""
import numpy as np
import pytest

from elim_cases import SMALL_CASES, case, dense_solve, eliminate

EPS = np.finfo(np.float64).eps


def scaled_diff(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("name", SMALL_CASES)
def test_the_elimination_is_the_dense_solve(name):
    c = case(name)
    cond = float(np.linalg.cond(c["M"]))
    assert cond < 1e4, "the case is meant to be well conditioned"
    for adjoint in (False, True):
        Y = eliminate(c["Jd"], c["p"], c["B"], adjoint)
        d = scaled_diff(Y, c["ref"][adjoint])
        print(name, "adjoint" if adjoint else "forward", "cond", cond, "difference", d, "bar", 64 * cond * EPS, "levels", c["plan"]["n_levels"])
        assert d <= 64 * cond * EPS, (name, adjoint, d)


def test_the_dense_solutions_solve_MM():
    c = case("three_level_12x6")
    N, nc, D = c["B"].shape
    for adjoint in (False, True):
        M = c["M"].T if adjoint else c["M"]
        r = M @ c["ref"][adjoint].transpose(0, 2, 1).reshape(N * D, nc) - c["B"].transpose(0, 2, 1).reshape(N * D, nc)
        assert np.max(np.abs(r)) <= 1e-12


@pytest.mark.parametrize("name,adjoint,defect", [("tdb_order1", False, "drop_next_half"), ("tdb_order1", True, "drop_next_half"),
                                                 ("three_level_12x6", False, "list_order"), ("three_level_12x6", True, "list_order"),
                                                 ("scaled_12x9", False, "list_order"), ("three_level_12x6", True, "adjoint_reads_deps"),
                                                 ("scaled_12x9", True, "adjoint_reads_deps")])
def test_the_bar_can_fail(name, adjoint, defect):
    c = case(name)
    d = scaled_diff(eliminate(c["Jd"], c["p"], c["B"], adjoint, defect=defect), c["ref"][adjoint])
    print(name, adjoint, defect, "difference", d)
    assert d > 1e-6, (name, defect, d)


def test_the_next_knot_half_matters_only_where_the_integrator_reaches_it():
    """spline order 0 holds the controls over the interval: dropping the k + 1 half changes nothing there"""
    c = case("tdb_order0")
    cond = float(np.linalg.cond(c["M"]))
    for adjoint in (False, True):
        d = scaled_diff(eliminate(c["Jd"], c["p"], c["B"], adjoint, defect="drop_next_half"), c["ref"][adjoint])
        assert d <= 64 * cond * EPS
