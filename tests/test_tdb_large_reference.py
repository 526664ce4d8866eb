"""CPU: the fast reference of tests/tdb_large_cases.py equals `O.OracleEvaluator` where the oracle is affordable (8 and 24
states), at the project's TimeDependentBilinearIntegrator bars (tests/test_gpu_time_dependent.py): 1e-10 relative for values and
Jacobian, 1e-8 for the Hessian.  This is what lets tests/test_gpu_time_dependent_large.py use the helper as its reference at
65..256 states, where the oracle's numerically differentiated Hessian does not finish."""
import numpy as np
import pytest

import dto_oracle as O
import tdb_large_cases as L
from helpers import rel_err


@pytest.mark.parametrize("n,order", [(8, 0), (8, 1), (24, 0), (24, 1)])
def test_fast_reference_equals_the_oracle(n, order):
    po = O.make_tdb_problem(N=3, n=n, m=2, order=order, seed=40 + n, substeps=8)
    ev_o = O.OracleEvaluator(po)
    ev_f, mu, g, j, h = L.reference(po, ("pin", n, order))
    assert np.array_equal(ev_f.jac_rows, ev_o.jac_rows) and np.array_equal(ev_f.jac_cols, ev_o.jac_cols)
    assert np.array_equal(ev_f.hess_rows, ev_o.hess_rows) and np.array_equal(ev_f.hess_cols, ev_o.hess_cols)
    Z = po.Z0
    errs = (rel_err(g, ev_o.eval_constraint(Z)), rel_err(j, ev_o.eval_constraint_jacobian(Z)),
            rel_err(h, ev_o.eval_hessian_lagrangian(Z, 0.6, mu)))
    print("fast reference vs oracle", n, order, errs)
    assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-8, errs


def test_fast_reference_with_a_derivative_integrator_between_the_blocks():
    """with_derivative=True puts other components and rows between the integrator's: the helper keeps the oracle's handling."""
    po = O.make_tdb_problem(N=3, n=8, m=2, order=1, seed=3, substeps=8, with_derivative=True)
    ev_o = O.OracleEvaluator(po)
    ev_f, mu, g, j, h = L.reference(po, ("pin-der", 8, 1))
    Z = po.Z0
    assert rel_err(g, ev_o.eval_constraint(Z)) <= 1e-10 and rel_err(j, ev_o.eval_constraint_jacobian(Z)) <= 1e-10
    assert rel_err(h, ev_o.eval_hessian_lagrangian(Z, 0.6, mu)) <= 1e-8
