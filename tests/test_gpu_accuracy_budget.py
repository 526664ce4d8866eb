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
last_stats() and the sweep forms, so that a failure names its interval and the form that ran.

Fixtures by state count: 9, 40, 66, 16 x 4 (structured), and -- with 16 sampled columns per E_k block (tests/hp_cases.py) -- 130
(npad 192: the chain's 64-tile GEMM three tiles a side, step-launch sweeps), 250 (npad 256: the ring GEMM on 2 x 2 tiles, once with
sub-stepped sweeps and the non-pairing Hessian, once with every sweep in one round: generator-stationary form, pairing Hessian)
and 330 (npad 384: the ring GEMM's 3 x 3 walk, step-launch sweeps beside the chain).  Which GEMM kernel those sizes get is pinned
on the CPU (tests/test_bgemm_dispatch_header.py); rounds and sweep forms are asserted here from last_stats() and the counters."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import hp_cases as C
from helpers import sweep_forms, to_engine

pytestmark = pytest.mark.gpu

NAMES = list(C.CASES)


def _callbacks(ev, fix):
    """The three callbacks; (outputs, last_stats() after each, the sweep forms each took)."""
    Z = fix["Z"]
    got, stats, forms = {}, {}, {}
    before = sweep_forms(ev)

    def note(cb):
        nonlocal before
        stats[cb] = ev.last_stats()
        now = sweep_forms(ev)
        forms[cb] = {f: now[f] - before[f] for f in now}
        before = now
    got["cons"] = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(got["cons"], Z)
    note("cons")
    got["jac"] = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(got["jac"], Z)
    note("jac")
    got["hess"] = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(got["hess"], Z, 0.0, fix["mu"])
    note("hess")
    return got, stats, forms


def _products(ev, fix, pad=0):
    """J w and J' w; `pad` extra constraint rows of the handle take weight 0 and are cut off."""
    y = np.full(ev.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, fix["Z"], fix["w"])
    wt = np.concatenate([fix["wt"], np.zeros(pad)])
    t = np.full(ev.n_variables, np.nan); ev.eval_constraint_jacobian_transpose_product(t, fix["Z"], wt)
    return dict(Jw=y[:y.size - pad] if pad else y, JTw=t)


@functools.lru_cache(maxsize=None)
def run_with(name, sweep_form=0):
    """One handle per fixture (and value of the option "sweep_form"), each callback once:
    (fixture, {(class, k): error}, text, {callback: last_stats()}, {callback: {form: sweeps}})."""
    fix = C.load(name)
    p, _ = C.at_point(name, fix["Z"])
    ev = dto_amd.Evaluator(to_engine(p), **C.ENGINE_KW.get(name, {}))
    try:
        if sweep_form:
            ev.set_option("sweep_form", sweep_form)
        ev.profile_enable()
        ev.profile_reset()
        got, stats, by_callback = _callbacks(ev, fix)
        got.update(_products(ev, fix))
        forms = sweep_forms(ev)
        route = {k: ev.profile_get(k)[1] for k in ("jac_product", "zero_fill")}
    finally:
        ev.close()
    errs = C.errors(name, fix, got)
    text = C.report(name, fix, errs, f"engine vs fixture{', sweep_form=1' if sweep_form else ''}: last_stats={stats['jac']} "
                    f"sweep_forms={forms} launches={route}\n  per callback: last_stats={stats} sweep_forms={by_callback}")
    print(text)
    return fix, errs, text, stats, by_callback


def run(name):
    return run_with(name)[:3]


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


@pytest.mark.parametrize("name", ["hp_general", "hp_ring256"])
def test_general_path_hessian_on_the_chains_plan(name):
    """reuse_forward_sweep = 1 and a Jacobian at the same point first: the Hessian's sweeps then take the step budget the
    propagator chain planned from its exact norms in place of the cheap bound."""
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
    _assert_within(name, errs, text, {"E", "dt", "const", "hess", "hess_outside_blocks"} | {f"u{j}" for j in range(C.CASES[name]["m"])})


# ---- what ran: the new fixtures are there for kernels and branches, so each run shows that it reached them -------------------------

SAMPLED = [n for n in NAMES if "sample_E" in C.CASES[n]]
ONE_ROUND = ["hp_ring256_q1"]
STEP_ONLY = ["hp_tile192", "hp_ring384"]


def terms_one_round_needs(r):
    """The fewest Taylor terms one round of radius r = ||A_k||_2 can end on.  last_stats()[1] is the largest number of terms a
    column block summed in ONE round (the engine reports no round count) -- as a running maximum over the callbacks of a handle
    that only a Jacobian call sets back to zero: after a Jacobian and a Hessian it is the larger of the two, so it bounds the
    Hessian's own count from above only.  "Fewer than one round needs" may therefore be read off it for the Hessian, "as many as
    one round needs" may not: that is read on a handle whose first call is the Hessian (hessian_alone).
    A_k is skew, hence normal: a column v with component c
    along the eigenpair of |lambda| = r has ||A^t v|| / t! >= |c| r^t / t!, and the termination test (two successive terms below
    1.1e-16 of the sum, whose norm is 1 here) cannot pass before that is below 1.1e-16.  x_k has 250..330 random entries, |c| is
    1 / sqrt(n) ~ 0.06 typically; 1e-3 is allowed for.  q rounds of radius r / q end near the count of r / q instead (with
    |c| = 1: the most it can be), which is far less: 28 terms for two rounds at r = 6 against 36, 46 and 59 for three and two
    rounds at r = 24 against 89."""
    t, term = 1, float(r)
    while term > 1.1e-16 / 1e-3:
        t += 1
        term *= r / t
    return t


def test_terms_rule_separates_one_round_from_several():
    assert terms_one_round_needs(6.0) == 36 and terms_one_round_needs(3.0) + 6 < 36
    assert terms_one_round_needs(24.0) == 89 and terms_one_round_needs(12.0) + 6 < 89


@functools.lru_cache(maxsize=None)
def hessian_alone(name, sweep_form=0):
    """A fresh handle whose only call is the Hessian: last_stats() then counts the Hessian's own sweeps (the forward column and
    the adjoint sweep), with no Jacobian's count carried over.  (last_stats(), {form: sweeps}, {(class, k): error}, text)."""
    fix = C.load(name)
    p, _ = C.at_point(name, fix["Z"])
    ev = dto_amd.Evaluator(to_engine(p), **C.ENGINE_KW.get(name, {}))
    try:
        if sweep_form:
            ev.set_option("sweep_form", sweep_form)
        ev.profile_enable()
        ev.profile_reset()
        h = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(h, fix["Z"], 0.0, fix["mu"])
        stats, forms = ev.last_stats(), sweep_forms(ev)
    finally:
        ev.close()
    errs = C.errors(name, fix, dict(hess=h))
    text = C.report(name, fix, errs, f"engine, the Hessian alone{', sweep_form=1' if sweep_form else ''}: last_stats={stats} sweep_forms={forms}")
    print(text)
    return stats, forms, errs, text


@pytest.mark.parametrize("name", SAMPLED)
def test_new_fixtures_run_the_rounds_and_forms_they_are_there_for(name):
    fix, errs, text, stats, forms = run_with(name)
    need = terms_one_round_needs(float(fix["norm2"].max()))
    terms = {cb: s[1] for cb, s in stats.items()}
    total = {f: sum(forms[cb][f] for cb in forms) for f in forms["cons"]}
    if name in ONE_ROUND:
        # one round in every callback: the generator-stationary form in each, which choose_sweep gives to q == 1 alone (in the
        # Hessian every one of its sweeps); values and Jacobian by their own term counts, the Hessian by its count on its own handle
        assert all(forms[cb]["gs"] >= 1 for cb in ("cons", "jac", "hess")), text
        assert all(forms[cb][f] == 0 for cb in forms for f in forms[cb] if f != "gs"), text
        assert terms["cons"] >= need and terms["jac"] >= need, (terms, need, text)
        h_stats, h_forms, h_errs, h_text = hessian_alone(name)
        assert h_stats[1] >= need, (h_stats, need, h_text)
        _assert_within(name, h_errs, h_text, {"hess", "hess_outside_blocks"})
    else:
        assert all(0 < t < need for t in terms.values()), (terms, need, text)
        assert total["gs"] == 0, text
    if name in STEP_ONLY:
        assert total["step"] >= 1 and all(total[f] == 0 for f in total if f != "step"), text
    assert stats["jac"][0] >= 1, text       # the chain squared: the top rungs are outside its radius


def test_step_launches_at_256_states_stay_within_the_budgets():
    """hp_ring256_q1 once more with sweep_form = 1: every sweep on one launch per Taylor step (k_sweep; with seven knots its
    32 x 32 tile, sweep_step_tile_rows), one round each, against the same bars."""
    name = "hp_ring256_q1"
    fix, errs, text, stats, forms = run_with(name, sweep_form=1)
    total = {f: sum(forms[cb][f] for cb in forms) for f in forms["cons"]}
    assert total["step"] >= 3 and all(total[f] == 0 for f in total if f != "step"), text
    assert all(forms[cb]["step"] >= 1 for cb in forms), text
    need = terms_one_round_needs(float(fix["norm2"].max()))
    assert stats["cons"][1] >= need and stats["jac"][1] >= need, (stats, need, text)
    # the Hessian's own count: on a handle of its own, where no Jacobian's count is carried over
    h_stats, h_forms, h_errs, h_text = hessian_alone(name, sweep_form=1)
    assert h_forms["step"] >= 1 and all(h_forms[f] == 0 for f in h_forms if f != "step"), h_text
    assert h_stats[1] >= need, (h_stats, need, h_text)
    _assert_within(name, h_errs, h_text, {"hess", "hess_outside_blocks"})
    m = C.CASES[name]["m"]
    _assert_within(name, errs, text, {"defect", "E", "dt", "const", "Jw", "JTw", "hess", "hess_outside_blocks"} | {f"u{j}" for j in range(m)})
