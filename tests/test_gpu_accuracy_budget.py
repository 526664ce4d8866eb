"""GPU: the exponential's accuracy budget, held to the 320-bit fixtures tests/golden/hp_*.npz (not to the fp64 oracle).

The metric is the normwise error per interval and quantity class (tests/hp_cases.py).  The bars come from the design, not from
any measurement of the engine: csrc/dto_sweep_plan.h plans the fewest sub-step rounds whose Taylor sums cannot lose more than
theta_v = 9 e-folds to cancellation, so a value, a Jacobian class, J w and J' w may be off by e^9 2^-53,
doubled for the accumulation over the rounds and the termination test at 1.1e-16: 2 e^9 2^-53 ~ 1.8e-12.  The Hessian pairs a
forward quantity with an adjoint one, each within that budget, and its second-order columns carry the same hump rule; to first
order the budgets add: 4 e^9 2^-53 ~ 3.6e-12 per interval block.  Inside the chain's radius (||A||_2 = 0.5) no squaring runs and
the last product stores -E_k: 64 2^-53 there.

Each interval of a fixture sits on another rung: no squaring, the chain's radii, one round, the q = 1 -> 2 switch of the hump
rule, several rounds.  Every callback runs once per handle into NaN-filled outputs; errors print per interval beside ||A_k||_2,
last_stats() and the sweep forms, so that a failure names its interval and the form that ran."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import hp_cases as C
from helpers import sweep_forms, to_engine

pytestmark = pytest.mark.gpu

NAMES = list(C.CASES)


def _callbacks(ev, fix, hessian=True):
    Z = fix["Z"]
    got = {}
    got["cons"] = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(got["cons"], Z)
    got["jac"] = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(got["jac"], Z)
    stats = ev.last_stats()
    if hessian:
        got["hess"] = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(got["hess"], Z, 0.0, fix["mu"])
    return got, stats


def _products(ev, fix, pad=0):
    """J w and J' w; `pad` extra constraint rows of the handle take weight 0 and are cut off."""
    y = np.full(ev.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, fix["Z"], fix["w"])
    wt = np.concatenate([fix["wt"], np.zeros(pad)])
    t = np.full(ev.n_variables, np.nan); ev.eval_constraint_jacobian_transpose_product(t, fix["Z"], wt)
    return dict(Jw=y[:y.size - pad] if pad else y, JTw=t)


@functools.lru_cache(maxsize=None)
def run(name):
    """One handle per fixture, each callback once: (fixture, {(class, k): error}, text)."""
    fix = C.load(name)
    p, _ = C.at_point(name, fix["Z"])
    ev = dto_amd.Evaluator(to_engine(p), **C.ENGINE_KW.get(name, {}))
    try:
        ev.profile_enable()
        ev.profile_reset()
        got, stats = _callbacks(ev, fix)
        got.update(_products(ev, fix))
        forms = sweep_forms(ev)
        route = {k: ev.profile_get(k)[1] for k in ("jac_product", "zero_fill")}
    finally:
        ev.close()
    errs = C.errors(name, fix, got)
    text = C.report(name, fix, errs, f"engine vs fixture: last_stats={stats} sweep_forms={forms} launches={route}")
    print(text)
    return fix, errs, text


def _assert_within(name, errs, text, classes):
    bad = [(cls, k, v, C.bar_for(cls)) for (cls, k), v in sorted(errs.items()) if cls in classes and not v <= C.bar_for(cls)]
    assert not bad, f"{name}: over the bar (class, interval, error, bar): {bad}\n{text}"


@pytest.mark.parametrize("name", NAMES)
def test_values_and_jacobian_classes_stay_within_the_sweep_budget(name):
    fix, errs, text = run(name)
    m = C.CASES[name]["m"]
    _assert_within(name, errs, text, {"defect", "E", "dt", "const"} | {f"u{j}" for j in range(m)})


@pytest.mark.parametrize("name", NAMES)
def test_matrix_free_products_stay_within_the_sweep_budget(name):
    fix, errs, text = run(name)
    _assert_within(name, errs, text, {"Jw", "JTw"})


@pytest.mark.parametrize("name", NAMES)
def test_hessian_blocks_stay_within_the_paired_budget(name):
    fix, errs, text = run(name)
    _assert_within(name, errs, text, {"hess", "hess_outside_blocks"})


@pytest.mark.parametrize("name", NAMES)
def test_propagator_inside_the_radius_is_good_to_a_few_ulps(name):
    fix, errs, text = run(name)
    k = int(np.argmin(fix["norm2"]))
    assert abs(fix["norm2"][k] - 0.5) < 1e-9
    assert errs[("E", k)] <= C.BAR_NO_SQUARING, f"{name}: E_{k} at ||A||_2 = 0.5: {errs[('E', k)]:.2e}\n{text}"


def _with_external_row(p):
    """The same problem with one closure constraint row behind the dynamics rows: an external constraint keeps a handle's
    J w / J' w on the value-slab route (include/dto_engine.h), as the existing product tests choose it."""
    u0 = p.integrators[0].u_off
    con = O.ClosureKnotConstraint(lambda v, q: np.array([v[0] * v[0] - 1.0]), lambda v, q: np.array([[2.0 * v[0]]]),
                                  lambda v, q, mu: np.array([[2.0 * mu[0]]]), [u0], [2], 1, equality=False)
    p.constraints = [con]
    return p


@pytest.mark.parametrize("name", NAMES)
def test_slab_route_products_stay_within_the_sweep_budget(name):
    fix = C.load(name)
    p, _ = C.at_point(name, fix["Z"])
    ev = dto_amd.Evaluator(to_engine(_with_external_row(p), closure_derivatives="analytic"), **C.ENGINE_KW.get(name, {}))
    try:
        ev.profile_enable()
        ev.profile_reset()
        got = _products(ev, fix, pad=1)
        route = {k: ev.profile_get(k)[1] for k in ("jac_product", "zero_fill")}
        stats = ev.last_stats()
    finally:
        ev.close()
    errs = C.errors(name, fix, got)
    text = C.report(name, fix, errs, f"engine (slab route) vs fixture: last_stats={stats} launches={route}")
    print(text)
    assert route["jac_product"] == 0 and route["zero_fill"] >= 1, route   # the slab was formed and contracted
    _assert_within(name, errs, text, {"Jw", "JTw"})


def test_general_path_hessian_on_the_chains_plan():
    """reuse_forward_sweep = 1 and a Jacobian at the same point first: the Hessian's sweeps then take the step budget the
    propagator chain planned from its exact norms in place of the cheap bound."""
    name = "hp_general"
    fix = C.load(name)
    p, _ = C.at_point(name, fix["Z"])
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        ev.set_option("reuse_forward_sweep", 1)
        ev.profile_enable()
        ev.profile_reset()
        j = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(j, fix["Z"])
        stats = ev.last_stats()
        h = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(h, fix["Z"], 0.0, fix["mu"])
        forms = sweep_forms(ev)
    finally:
        ev.close()
    errs = C.errors(name, fix, dict(jac=j, hess=h))
    text = C.report(name, fix, errs, f"engine, reuse_forward_sweep=1: last_stats={stats} sweep_forms={forms}")
    print(text)
    _assert_within(name, errs, text, {"E", "u0", "dt", "const", "hess", "hess_outside_blocks"})
