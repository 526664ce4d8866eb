"""CPU: the dense reference of the reduced-space operators (reduced_cases.dense_reference) on its own, from the oracle alone.

1. It is the derivative of the reduced gradient along the feasible manifold: <d2, Hr d1> against the central difference of
   <d2, r_ref(feasible(Z* +- h d1))>, h = 1e-5, three pairs of directions, relative <= 1e-6 -- the project's step and bar.
2. The bar of the GPU tests can fail: three named mistakes in the multipliers of the dynamics rows (zero; +Lam instead of -Lam; Lam
   shifted by one knot) miss y_ref by at least 1000 x that bar.
3. The condition on the inputs: kappa <= 1e4, so the bar never exceeds 1e-4 relative."""
import numpy as np
import pytest

import reduced_cases as R


@pytest.mark.parametrize("name", R.SMALL_CASES)
def test_the_dense_reference_against_central_differences_along_the_feasible_manifold(name):
    c = R.case(name)
    p, mu = c["p"], c["mu"]
    Zs = R.oracle_feasible(p, c["Z"])
    assert np.max(np.abs(np.concatenate([R.O.integrator_evaluate(it, p, Zs) for it in p.integrators]))) <= 1e-12
    ref = R.dense_reference(p, Zs, R.SIGMA, mu)
    rng = np.random.default_rng(23)
    h = 1e-5
    for trial in range(3):
        d1, d2 = R.free_direction(p, rng), R.free_direction(p, rng)
        an = float(d2 @ R.product_ref(ref, d1))
        rp = R.reduced_gradient_ref(p, R.oracle_feasible(p, Zs + h * d1), R.SIGMA, mu)
        rm = R.reduced_gradient_ref(p, R.oracle_feasible(p, Zs - h * d1), R.SIGMA, mu)
        fd = float(d2 @ (rp - rm)) / (2.0 * h)
        rel = abs(an - fd) / max(abs(an), abs(fd))
        print(name, "pair", trial, "analytic", an, "central difference", fd, "relative", rel)
        assert rel <= 1e-6, (name, trial, rel)


@pytest.mark.parametrize("name", R.SMALL_CASES)
@pytest.mark.parametrize("mistake", ["zero", "plus", "shift"])
def test_a_named_mistake_in_the_dynamics_multipliers_misses_the_bar_a_thousandfold(name, mistake):
    c = R.case(name)
    wrong = R.dense_reference(c["p"], c["Z"], R.SIGMA, c["mu"], mistake=mistake)
    for v, y in zip(c["vs"], c["ys"]):
        miss, limit = float(np.linalg.norm(R.product_ref(wrong, v) - y)), R.product_bar(c["ref"], v)
        print(name, mistake, "misses by", miss, "bar", limit, "ratio", miss / limit)
        assert miss >= 1000.0 * limit, (name, mistake, miss / limit)


@pytest.mark.parametrize("name", R.SMALL_CASES)
def test_the_cases_are_well_conditioned_and_the_reference_is_symmetric(name):
    c = R.case(name)
    ref = c["ref"]
    for v in c["vs"]:
        k = R.kappa(ref, v)
        print(name, "kappa", k, "||T||", ref["nT"], "||H||", ref["nH"], "||g||", ref["ng"])
        assert k <= R.KAPPA_CAP
    assert np.max(np.abs(ref["Hr"] - ref["Hr"].T)) <= 1e-12 * ref["nT"] ** 2 * ref["nH"]
    assert np.all(c["ref"]["r_ref"][ref["S"]] == 0.0)
