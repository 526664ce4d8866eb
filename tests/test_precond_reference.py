"""CPU, oracle only: the restated L-BFGS preconditioner (precond_cases.py, which test_precond_plan_header.py holds csrc/dto_precond_plan.h
to) on the ORACLE's dense reduced Hessian and gradient, with the shift of newton_box_cases.small_scenarios.

The application is judged by a textbook two-loop recursion run in np.longdouble.  The bar is not a fixed number: per case the
double-precision two-loop's own error against the longdouble one is measured, and the compact form gets that error times a margin of
8, for the two triangular solves it adds.  The pairs are the last 8 CG pairs of a plain solve, as a harvest leaves them."""
import functools

import numpy as np
import pytest

import newton_box_cases as B
import precond_cases as PC
import reduced_cases as R
from newton_box_cases import CONVERGED, FREE, HIT_LO
from test_gpu_newton_step import dense_bar

CASES = ["scaled_12x9", "scaled_12x9+con", "scaled_40x6", "tdb_order1"]
MARGIN = 8.0


@functools.lru_cache(maxsize=None)
def solves(name, scenario="inf", rtol=None):
    """a plain solve with harvest, and the solve at the same point preconditioned with its last 8 pairs"""
    c, sc = R.case(name), B.small_scenarios(name)
    kw = dict(sc[scenario]) if rtol is None else dict(sc[scenario], rtol=rtol)
    g, nonfixed, prod = np.array(c["ref"]["r_ref"]), B.nonfixed_of(c["p"]), B.oracle_product(name)
    plain = PC.precond_loop(prod, g, nonfixed, c["Z"], harvest=True, **kw)
    pairs = plain["pairs"][-8:]
    S, Y = [d for d, _ in pairs], [w for _, w in pairs]
    pre = PC.precond_loop(prod, g, nonfixed, c["Z"], S, Y, **kw)
    return dict(c=c, sc=sc, kw=kw, g=g, nonfixed=nonfixed, plain=plain, pre=pre, S=S, Y=Y)


def relative(a, b):
    return float(np.linalg.norm((np.asarray(a, dtype=np.longdouble) - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


@pytest.mark.parametrize("name", CASES)
def test_the_compact_form_against_a_two_loop_recursion_in_longdouble(name):
    s = solves(name)
    S, Y, F = s["S"], s["Y"], s["nonfixed"]
    assert len(S) == 8 and all(np.all(d[~F] == 0.0) and np.all(w[~F] == 0.0) for d, w in zip(S, Y)), "CG pairs vanish outside F0"
    P = PC.prepare_restated(S, Y, F)
    assert P["idx"] == list(range(8)), "every CG pair is admitted"
    r = np.where(F, s["g"], 0.0)
    exact = PC.two_loop(S, Y, r, np.longdouble)
    own = relative(PC.two_loop(S, Y, r, np.float64), exact)
    err = relative(PC.apply_restated(P, r, F)[0], exact)
    print(name, "gradient: two-loop in double against longdouble", own, "compact form", err, "ratio", err / own)
    assert own > 0.0 and err <= MARGIN * own
    # the secant equation of the newest pair, H y~_k = s~_k.  The two-loop recursion meets it exactly in any precision (its first step
    # cancels y_k against itself), so it has no error of its own to measure there: the bar is the case's bar above.
    assert relative(PC.two_loop(S, Y, Y[-1], np.longdouble), S[-1].astype(np.longdouble)) <= 1e-18
    secant = relative(PC.apply_restated(P, Y[-1], F)[0], S[-1].astype(np.longdouble))
    print(name, "secant: ||H y_k - s_k|| / ||s_k||", secant, "ratio", secant / own)
    assert secant <= MARGIN * own


@pytest.mark.parametrize("name", CASES)
def test_harvested_pairs_save_iterations_at_the_same_point(name):
    s = solves(name)
    plain, pre = s["plain"]["info"], s["pre"]["info"]
    print(name, "plain", int(plain[1]), "preconditioned", int(pre[1]), "admitted", int(pre[12]), "fallbacks", int(pre[14]))
    assert plain[0] == pre[0] == CONVERGED and pre[12] == 8 and pre[14] == 0
    assert pre[1] < plain[1], "strictly fewer iterations"
    box = B.box_loop(B.oracle_product(name), s["g"], s["nonfixed"], s["c"]["Z"], **s["kw"])
    assert np.array_equal(s["plain"]["p"], box["p"]) and np.array_equal(plain[:12], box["info"]), "with an empty store the loop is the box loop"


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("scenario", ("inf",) + B.CONVEX)
def test_the_converged_solution_against_the_dense_solve(name, scenario):
    """On the final face ||p_F - solve(A_FF, -(g_F + A_FB p_B))|| <= (2 rtol ||g|| + gradient_bar + product_bar(p)) / lambda_min(A_FF): the bar
    of test_gpu_newton_box.test_values_against_the_oracle (its gradient and product terms are the engine's allowances; the restated loop on
    the oracle's matrix has less to spend).  The convergence test stays Euclidean under preconditioning, so the bar is the same."""
    s = solves(name, scenario, 1e-10)
    c, got = s["c"], s["pre"]
    ref, Cidx = c["ref"], c["ref"]["C"]
    assert got["info"][0] == CONVERGED and got["info"][12] >= 1
    es, x = got["states"][Cidx], got["p"][Cidx]
    F, Bd = es == FREE, es >= HIT_LO
    A = ref["Hr"] + s["sc"]["shift"] * np.eye(Cidx.size)
    g = ref["r_ref"][Cidx]
    pF = np.linalg.solve(A[np.ix_(F, F)], -(g[F] + A[np.ix_(F, Bd)] @ x[Bd]))
    err = float(np.linalg.norm(x[F] - pF))
    b = dense_bar(ref, c["levels"], 1e-10, A[np.ix_(F, F)], got["p"], float(got["info"][2]))
    print(name, scenario, "iterations", int(got["info"][1]), "plain", int(s["plain"]["info"][1]), "free", int(F.sum()), "hit", int(Bd.sum()),
          "||p_F - p_F*||", err, "bar", b, "ratio", err / b)
    assert err <= b
    kw = s["kw"]
    if "lo" in kw:
        assert np.all(got["Zp"][Cidx] >= kw["lo"][Cidx]) and np.all(got["Zp"][Cidx] <= kw["hi"][Cidx]), "inside the box, exactly"
