"""CPU: the sparse reference of the long-horizon tests (long_cases.py) on its own, from the oracle alone.

1. It IS the reference the suite already trusts: on every SMALL_CASES entry of reduced_cases and elim_cases it reproduces the dense one --
   r_ref, Hr v for the case's two directions, both solves -- to 1e-11 in the units of the dense bar (the bar's formula with 1e-11 in the
   place of its tolerance; rel_err <= 1e-11 for the solves).  Both references run a backward-stable LU on the same matrices, so they
   differ by a modest multiple of eps cond(J_S) <= 1.1e-16 x 1.5e3 = 1.7e-13 in those units: 1e-11 leaves a factor 60.
2. Every long case meets its conditions with the reference alone: kappa <= KAPPA_CAP for every direction the values tests use, and the
   reference's own error -- the change one step of iterative refinement with a np.longdouble residual makes -- is under 1/100 of the
   bar it is used with.  The numbers are printed.
3. The bar can fail at length: at scaled_12x258 the named mistakes "zero" and "plus" of reduced_cases.dense_reference, restated for the
   sparse reference, miss y_ref by at least 1000 x product_bar (measured: 3.2e4 .. 9.9e4 x).  The third, "shift", does NOT reach the
   factor at this length and is left out: 257 intervals share the span of 3, so neighbouring knots' multipliers differ little and
   the shifted ones miss by 1.0e3 x and 3.7e2 x the bar on the case's two directions.  The factor is unchanged."""
import numpy as np
import pytest

import elim_cases as E
import long_cases as L
import reduced_cases as R
from helpers import rel_err
from test_gpu_rollout import bar


# --------------------------------------------------------------------------------------------- 1. the tie to the dense reference
@pytest.mark.parametrize("name", R.SMALL_CASES)
def test_the_sparse_reference_reproduces_the_dense_reduced_reference(name):
    c = R.case(name)
    d = c["ref"]
    s = L.sparse_reference(c["p"], c["Z"], R.SIGMA, c["mu"])
    print(name, "||T||", s["nT"], d["nT"], "||H||", s["nH"], d["nH"], "||g||", s["ng"], d["ng"])
    assert abs(s["nT"] - d["nT"]) <= 1e-6 * d["nT"] and abs(s["nH"] - d["nH"]) <= 1e-6 * d["nH"] and abs(s["ng"] - d["ng"]) <= 1e-12 * d["ng"]
    assert np.array_equal(s["S"], d["S"]) and np.array_equal(s["C"], d["C"])
    eg, ug = float(np.linalg.norm(s["r_ref"] - d["r_ref"])), d["nT"] ** 2 * d["ng"]
    print(name, "gradient: sparse - dense", eg, "in the bar's units", eg / ug)
    assert eg <= 1e-11 * ug
    el = float(np.linalg.norm(s["lam"] - d["lam"]))
    assert el <= 1e-11 * d["nT"] * d["ng"], ("lam", el)
    for v, y in zip(c["vs"], c["ys"]):
        e, u = float(np.linalg.norm(L.product_ref(s, v) - y)), d["nT"] ** 2 * d["nH"] * float(np.linalg.norm(v[d["C"]]))
        print(name, "product: sparse - dense", e, "in the bar's units", e / u, "kappa sparse, dense", L.kappa(s, v), R.kappa(d, v))
        assert e <= 1e-11 * u
        assert np.all(L.product_ref(s, v)[d["S"]] == 0.0)


@pytest.mark.parametrize("name", E.SMALL_CASES)
def test_the_sparse_solve_reproduces_the_dense_solve(name):
    c = E.case(name)
    MM = L.sparse_MM(L.sparse_jacobian(c["p"], c["Z"]), c["p"])
    assert MM.shape == c["M"].shape and np.array_equal(MM.toarray(), c["M"]), "the sparse MM is elim_cases.assemble entry for entry"
    F = L.Factor(MM)
    for adjoint in (False, True):
        e = rel_err(L.sparse_solve(F, c["B"], adjoint), c["ref"][1 if adjoint else 0])
        print(name, "adjoint" if adjoint else "forward", "sparse - dense", e)
        assert e <= 1e-11


# --------------------------------------------------------------------------------------- 2. the long cases meet their conditions
@pytest.mark.parametrize("name", L.LONG_CASES)
def test_a_long_case_is_well_conditioned_and_its_reference_is_a_hundredfold_below_the_bars(name):
    c = L.case(name)
    ref = c["ref"]
    print(name, "n_vars", c["p"].n_vars, "|C|", ref["C"].size, "||T||", ref["nT"], "||H||", ref["nH"], "||g||", ref["ng"], "cond_1(J_S)",
          ref["JS"].cond1(), "levels", c["levels"])
    eg, bg = float(np.linalg.norm(L.gradient_ref(ref, refine=True) - ref["r_ref"])), L.gradient_bar(ref, c["levels"])
    print(name, "gradient: the reference's error", eg, "bar", bg, "ratio", eg / bg)
    assert eg <= bg / 100.0
    for v, y in zip(c["vs"], c["ys"]):
        k, e, b = L.kappa(ref, v, y), float(np.linalg.norm(L.product_ref(ref, v, refine=True) - y)), L.product_bar(ref, v)
        print(name, "kappa", k, "product: the reference's error", e, "bar", b, "ratio", e / b)
        assert k <= L.KAPPA_CAP
        assert e <= b / 100.0
        assert np.all(y[ref["S"]] == 0.0)
    sym = np.random.default_rng(5).standard_normal((2, c["p"].n_vars))
    a, b2 = float(sym[0] @ L.product_ref(ref, sym[1])), float(sym[1] @ L.product_ref(ref, sym[0]))
    assert abs(a - b2) <= 1e-11 * ref["nT"] ** 2 * ref["nH"] * float(np.linalg.norm(sym[0]) * np.linalg.norm(sym[1])), "T' H T is symmetric"


@pytest.mark.parametrize("name", L.C1_CASES + [L.C2_CASE, L.C3_CASE])
def test_the_sparse_solves_own_error_is_a_hundredfold_below_the_bar(name):
    c = L.jac_case(name)
    K, limit = c["p"].N - 1, bar(c["p"].N - 1) * c["levels"]
    print(name, "K", K, "levels", c["levels"], "N D", c["MM"].A.shape[0], "cond_1(MM)", c["MM"].cond1(), "bar", limit)
    for adjoint in (False, True):
        Y = c["ref_solve"][1 if adjoint else 0]
        e = rel_err(L.sparse_solve(c["MM"], c["B"], adjoint, refine=True), Y)
        res = max(float(np.max(np.abs(c["MM"].residual(L.sparse_solve(c["MM"], c["B"], adjoint)[:, j].reshape(-1), c["B"][:, j].reshape(-1), adjoint))))
                  for j in range(c["B"].shape[1])) / float(np.max(np.abs(c["B"])))
        print(name, "adjoint" if adjoint else "forward", "the reference's error", e, "ratio", e / limit, "residual", res, "max |y|", float(np.max(np.abs(Y))))
        assert e <= limit / 100.0


# ------------------------------------------------------------------------------------------------- 3. the bar can fail at length
@pytest.mark.parametrize("mistake", ["zero", "plus"])
def test_a_named_mistake_in_the_dynamics_multipliers_misses_the_bar_a_thousandfold_at_length(mistake):
    c = L.case(L.MISTAKE_CASE)
    wrong = L.sparse_reference(c["p"], c["Z"], R.SIGMA, c["mu"], mistake=mistake, base=c["ref"])
    for v, y in zip(c["vs"], c["ys"]):
        miss, limit = float(np.linalg.norm(L.product_ref(wrong, v) - y)), L.product_bar(c["ref"], v)
        print(L.MISTAKE_CASE, mistake, "misses by", miss, "bar", limit, "ratio", miss / limit)
        assert miss >= 1000.0 * limit, (mistake, miss / limit)
