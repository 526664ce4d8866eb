"""The dense reference of the augmented-Lagrangian tests (auglag_cases.py) judged by the ORACLE alone, without a GPU: Phi, its reduced
gradient and Hr_AL = T'(H(sigma, [lam; mu_eff]) + J_c' W J_c)T are consistent with each other, the cases meet the condition the GPU bars
assume, and the outer loop of the README converges on al_12x9 -- which is what makes the comparison of the engine's run with it
(test_gpu_auglag.py) meaningful."""
import numpy as np
import pytest

import auglag_cases as A
import reduced_cases as R

SIGMA = A.SIGMA


def central(f, Z, d, h):
    return (f(Z + h * d) - f(Z - h * d)) / (2.0 * h)


@pytest.mark.parametrize("name", A.SMALL_CASES)
def test_the_gradient_is_the_derivative_of_phi(name):
    """central differences of Phi(oracle_feasible(.)) along two free directions at h = 1e-4 and 5e-5: second order, so the error falls
    by a factor between 3 and 5, or is below 1e-9 relative already"""
    c = A.case(name)
    p, Z, mu, rho, ref = c["p"], c["Z"], c["mu"], c["rho"], c["ref"]
    phi = lambda X: A.phi_ref(p, X, SIGMA, mu, rho)
    for seed in (1, 2):
        d = R.free_direction(p, np.random.default_rng(seed))
        d /= np.linalg.norm(d)
        exact = float(ref["r_ref"] @ d)
        e1, e2 = (abs(central(phi, Z, d, h) - exact) for h in (1e-4, 5e-5))
        print(name, seed, "g.d", exact, "errors", e1, e2, "ratio", e1 / e2 if e2 else np.inf)
        assert 3.0 <= e1 / e2 <= 5.0 or e2 <= 1e-9 * abs(exact)


@pytest.mark.parametrize("name", A.SMALL_CASES)
def test_the_product_is_the_derivative_of_the_gradient(name):
    """Hr_AL v against central differences of the reduced gradient of Phi along v; no row of the case has |s| below 1e-3, so no row
    changes sides within h"""
    c = A.case(name)
    p, Z, mu, rho, ref = c["p"], c["Z"], c["mu"], c["rho"], c["ref"]
    if name == "al_12x9":
        # A constraint whose `times` repeat a knot keeps only the later listing's Hessian block (the reference's block view is
        # overwritten, knot_point_constraint.jl:285-291), so H is no second derivative where such a row has a multiplier: its rows are
        # made inactive here (mult = 0, weight = 0), 0.5 away from the switch.
        rows = slice(c["n_cons"] - 3, c["n_cons"])
        mu = np.array(mu)
        mu[rows] = -A.RHO * A.constraint_values(p, Z)[-3:] - 0.5
        ref = A.dense_reference(p, Z, SIGMA, mu, rho)
        assert np.all(ref["weight"][-3:] == 0.0) and np.all(ref["mult"][-3:] == 0.0)
    Cidx = ref["C"]

    def grad(X):
        Xf = R.oracle_feasible(p, X)
        return A.dense_reference(p, Xf, SIGMA, mu, rho)["r_ref"][Cidx]

    d = R.free_direction(p, np.random.default_rng(4))
    d /= np.linalg.norm(d)
    exact = ref["Hr"] @ d[Cidx]
    e1, e2 = (float(np.linalg.norm(central(grad, Z, d, h) - exact)) for h in (1e-4, 5e-5))
    print(name, "|Hr v|", float(np.linalg.norm(exact)), "errors", e1, e2, "ratio", e1 / e2 if e2 else np.inf)
    assert 3.0 <= e1 / e2 <= 5.0 or e2 <= 1e-7 * float(np.linalg.norm(exact))
    assert np.allclose(ref["Hr"], ref["Hr"].T, rtol=0, atol=1e-9 * ref["nH"] * ref["nT"] ** 2), "symmetric"


@pytest.mark.parametrize("name", A.VALUE_CASES)
def test_the_cases_meet_the_condition_of_the_bars(name):
    c = A.case(name)
    ref = c["ref"]
    for seed in (1, 2):
        v = np.random.default_rng(seed).standard_normal(c["Z"].size)
        k = R.kappa(ref, v)
        print(name, "kappa", k, "||H_AL||", ref["nH"], "||T||", ref["nT"])
        assert k <= R.KAPPA_CAP
    assert 0.25 <= c["share"] <= 0.75
    assert np.any(ref["weight"] != 0.0) and np.any(ref["weight"] == 0.0), "active and inactive rows"


def test_penalised_rows_carry_the_largest_curvature():
    """the reason the step needs the term: on al_12x9 the Gauss-Newton part is no small correction of T'HT"""
    c = A.case("al_12x9")
    ref = c["ref"]
    plain = R.dense_reference(c["p"], c["Z"], SIGMA, c["mu_eff"])
    gn = float(np.linalg.norm(ref["Hr"] - plain["Hr"], 2))
    print("||T'HT||", float(np.linalg.norm(plain["Hr"], 2)), "||T' J_c' W J_c T||", gn)
    assert gn >= 0.1 * float(np.linalg.norm(plain["Hr"], 2))


def test_the_outer_loop_converges_on_al_12x9():
    """five outer iterations of ten trust-region trials with dense oracle operators: max viol from at least 0.1 to below 1e-4"""
    log = A.oracle_outer_run("al_12x9")
    print("max viol at the start", log["viol0"], "behind each outer iteration", log["viol"], "rho grew", log["grew"])
    print("accepted", log["accepted"])
    assert log["viol0"] >= 0.1
    assert log["viol"][-1] < 1e-4
    assert all(any(a) for a in log["accepted"]), "every inner loop moves"


def test_the_outer_loop_is_no_amplifier_of_rounding():
    """operators and merit values perturbed by 1e-13 relative leave every decision as it was and max viol within 1e-3 relative (measured: 1e-8 .. 4e-6): two
    implementations that differ by rounding can be held to one another's decisions"""
    base, pert = A.oracle_outer_run("al_12x9"), A.oracle_outer_run("al_12x9", 1e-13)
    assert pert["accepted"] == base["accepted"] and pert["grew"] == base["grew"]
    assert np.allclose(pert["viol"], base["viol"], rtol=1e-3, atol=0.0)
