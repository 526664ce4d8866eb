"""Shared by the tests of the reduced-space minimize call (dto_projected_minimize; csrc/dto_minimize_plan.h, csrc/dto_minimize.hip): the
header's rules restated in NumPy -- trial_decide, outer_decide and minimize_loop around ANY step, merit and row pass (the header's toy
callables, the oracle's dense operators, the engine's public methods) -- and the oracle-only runs the tests compare with, built from
reduced_cases, newton_box_cases and auglag_cases.

Every operation is one IEEE double operation, in the header's operand order, so the restatement has the header's bits."""
import functools
import math

import numpy as np

import auglag_cases as A
import newton_box_cases as B
import reduced_cases as R
from newton_box_cases import CONVERGED, NOT_FINITE

SIGMA = R.SIGMA
# exit status, inner stops
M_RUNNING, M_CONVERGED, M_MAX_OUTER, M_MAX_TRIALS, M_RADIUS, M_NOT_FINITE = -1, 0, 1, 2, 3, 4
STOP_NONE, STOP_GRADIENT, STOP_RADIUS, STOP_NOT_FINITE, STOP_MAX_TRIALS = 0, 1, 2, 3, 4
OPTIONS = ("radius0", "eta_accept", "eta_shrink", "eta_grow", "shrink_div", "grow_mul", "radius_max", "radius_min", "gtol", "ctol", "viol_div",
           "rho_mul", "shift", "rtol", "atol", "max_iter")
DEFAULTS = (1.0, 0.1, 0.25, 0.75, 4.0, 2.0, math.inf, 0.0, 0.0, 0.0, 4.0, 10.0, 0.0, 1e-6, 0.0, 50.0)
(O_RADIUS0, O_ACCEPT, O_SHRINK, O_GROW, O_SHRINK_DIV, O_GROW_MUL, O_RADIUS_MAX, O_RADIUS_MIN, O_GTOL, O_CTOL, O_VIOL_DIV, O_RHO_MUL, O_SHIFT, O_RTOL,
 O_ATOL, O_MAX_ITER) = range(16)
F64 = np.float64


def options(**kw):
    assert set(kw) <= set(OPTIONS), kw
    return np.array([float(kw.get(k, d)) for k, d in zip(OPTIONS, DEFAULTS)])


def step_kw(opt):
    """the step's keywords from the options"""
    return dict(shift=float(opt[O_SHIFT]), rtol=float(opt[O_RTOL]), atol=float(opt[O_ATOL]), max_iter=int(opt[O_MAX_ITER]))


# ------------------------------------------------------------------------------------------------------ the rules, restated
def trial_decide(phi, phi_t, predicted, step_status, delta, opt):
    """(ratio, accepted, delta_next, stop)"""
    with np.errstate(all="ignore"):
        ratio = float((F64(phi) - F64(phi_t)) / F64(predicted))
    if step_status == NOT_FINITE or not math.isfinite(ratio):
        return ratio, False, float(delta), STOP_NOT_FINITE
    accepted, delta_next = bool(ratio > opt[O_ACCEPT]), float(delta)
    if ratio < opt[O_SHRINK]:
        delta_next = float(F64(delta) / F64(opt[O_SHRINK_DIV]))
    elif ratio > opt[O_GROW] and step_status != CONVERGED:
        grown = float(F64(delta) * F64(opt[O_GROW_MUL]))
        delta_next = float(opt[O_RADIUS_MAX]) if opt[O_RADIUS_MAX] < grown else grown
    return ratio, accepted, delta_next, (STOP_RADIUS if delta_next < opt[O_RADIUS_MIN] else STOP_NONE)


def outer_decide(viol, new_viol, opt):
    """(grew, feasible)"""
    with np.errstate(all="ignore"):
        return (not new_viol <= float(F64(viol) / F64(opt[O_VIOL_DIV]))), bool(new_viol <= opt[O_CTOL])


def rho_next(rho, grew, opt):
    rho = np.asarray(rho, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.where(rho != 0.0, rho * opt[O_RHO_MUL], rho) if grew else rho.copy()


def minimize_loop(step, merit, rows, Z, mu, rho, n_dyn, opt=None, outer=1, trials=10, step_info=12):
    """minimize_solve of csrc/dto_minimize_plan.h.
        step(Z, delta, mu, rho) -> (info, Zp[, states])    info: the step's 12 or 16 doubles
        merit(Z, mu, rho) -> (phi, Zf)
        rows(Z, mu, rho) -> (mu_eff, raw)                   raw: the row pass's eight scalars
    Returns a dict: Z, mu, rho, info [16], history (trials run, 8), outer_history (row passes, 4), states (the last step's or None),
    accepted (per outer iteration the trials' decisions), iterates (the accepted Z of every trial) and merits (how many merit calls)."""
    opt = options() if opt is None else np.asarray(opt, dtype=np.float64)
    Z = np.array(Z, dtype=np.float64)
    has_rho = rho is not None
    mu = None if mu is None else np.array(mu, dtype=np.float64)
    rho = None if rho is None else np.array(rho, dtype=np.float64)
    s = np.zeros(16)                     # the scalars: info as it stands, the inner stop in [14]
    history, outer_history, accepted_log, iterates, states = [], [], [], [], None
    merits, launches = 0, 0
    viol0 = rows(Z, mu, rho)[1][2] if has_rho else 0.0
    status = M_RUNNING
    for o in range(outer if has_rho else 1):
        phi, Z = merit(Z, mu, rho)
        merits += 1
        Z = np.array(Z, dtype=np.float64)
        delta, stop, log = float(opt[O_RADIUS0]), STOP_NONE, []
        for t in range(trials):
            out = step(Z, delta, mu, rho)
            sinfo, Zp = np.asarray(out[0], dtype=np.float64), out[1]
            if len(out) > 2:
                states = out[2]
            gradient = bool(sinfo[2] <= opt[O_GTOL])
            if gradient:
                ratio, ok, delta_next, stop, phi_t = 0.0, False, delta, STOP_GRADIENT, phi
            else:
                phi_t, Zt = merit(Zp, mu, rho)
                merits += 1
                ratio, ok, delta_next, stop = trial_decide(phi, phi_t, sinfo[6], int(sinfo[0]), delta, opt)
            if stop == STOP_NONE and t == trials - 1:
                stop = STOP_MAX_TRIALS
            if launches == 0:
                s[4] = phi
            if t == 0:
                s[1] += 1.0
            history.append([ratio, float(ok), delta, phi_t, sinfo[6], sinfo[0], sinfo[1], sinfo[2]])
            s[2] += 1.0
            s[3] += float(ok)
            if ok:
                Z, phi = np.array(Zt, dtype=np.float64), phi_t
            s[5], s[6], s[7] = phi, delta_next, sinfo[2]
            s[11] += sinfo[1]
            if step_info >= 16:
                s[12] += sinfo[13]
                s[13] += sinfo[14]
            s[14] = stop
            status = M_RUNNING
            if stop == STOP_NOT_FINITE:
                status = M_NOT_FINITE
            elif not has_rho and stop != STOP_NONE:
                status = {STOP_GRADIENT: M_CONVERGED, STOP_RADIUS: M_RADIUS, STOP_MAX_TRIALS: M_MAX_TRIALS}[stop]
            s[0] = status
            launches += 1
            log.append(ok)
            iterates.append(Z.copy())
            delta = delta_next
            if stop != STOP_NONE:
                break
        accepted_log.append(log)
        if stop == STOP_NOT_FINITE or not has_rho:
            break
        mu_eff, raw = rows(Z, mu, rho)
        viol = viol0 if o == 0 else s[9]
        new_viol = float(raw[2])
        grew, feasible = outer_decide(viol, new_viol, opt)
        if o == 0:
            s[8] = viol0
        s[9] = new_viol
        s[10] += float(grew)
        status = M_CONVERGED if (stop == STOP_GRADIENT and feasible) else M_MAX_OUTER if o == outer - 1 else M_RUNNING
        s[0] = status
        outer_history.append([new_viol, float(grew), raw[1], raw[0]])
        mu[n_dyn:] = np.asarray(mu_eff)[n_dyn:]
        rho[n_dyn:] = rho_next(rho[n_dyn:], grew, opt)
        launches += 1
        if status != M_RUNNING:
            break
    info = s.copy()
    info[14] = 0.0
    return dict(Z=Z, mu=mu, rho=rho, info=info, history=np.array(history, dtype=np.float64).reshape(len(history), 8),
                outer_history=np.array(outer_history, dtype=np.float64).reshape(len(outer_history), 4), states=states, accepted=accepted_log,
                iterates=iterates, merits=merits, grew=[bool(r[1]) for r in outer_history], viol=[r[0] for r in outer_history], viol0=viol0)


# --------------------------------------------------------------------------------------------- the oracle-only runs
def oracle_callables(p, lo=None, hi=None, opt=None):
    """(step, merit, rows) of minimize_loop from the oracle's dense operators alone (auglag_cases.oracle_outer_run's, with the
    signatures of minimize_loop)"""
    opt = options() if opt is None else opt
    nonfixed = B.nonfixed_of(p)
    kw = step_kw(opt)

    def step(Z, delta, mu, rho):
        if rho is None:
            ref = R.dense_reference(p, Z, SIGMA, mu)
        else:
            ref = A.dense_reference(p, Z, SIGMA, mu, rho)
        out = B.box_loop(lambda d: R.product_ref(ref, d), np.array(ref["r_ref"]), nonfixed, Z, lo, hi, radius=delta, **kw)
        return out["info"], out["Zp"], out["states"]

    def merit(Zp, mu, rho):
        if rho is None:
            import dto_oracle as O
            Zf = R.oracle_feasible(p, Zp)
            ev_o = O.OracleEvaluator(p)
            phi = SIGMA * ev_o.eval_objective(Zf)
            if mu is not None:
                n_dyn = sum(it.x_dim for it in p.integrators) * (p.N - 1)
                phi += float(np.asarray(mu)[n_dyn:] @ ev_o.eval_constraint(Zf)[n_dyn:])
            return phi, Zf
        phi, Zf, _ = A.phi_ref(p, Zp, SIGMA, mu, rho, trajectory=True)
        return phi, Zf

    def rows(Z, mu, rho):
        n_dyn, (psi, mult, weight, viol) = A.rows_at(p, Z, mu, rho)
        raw = np.array([float(np.sum(psi)), float(np.sum(weight != 0.0)), float(np.max(viol)), 0.0, 0.0, 0.0, 0.0, 0.0])
        return A.full(n_dyn, mult), raw

    return step, merit, rows


@functools.lru_cache(maxsize=None)
def oracle_minimize_run(name="al_12x9", outer=5, trials=10):
    """auglag_cases.oracle_outer_run's problem, start and settings through minimize_loop"""
    c = A.case(name, dense=False)
    opt = options(**A.STEP_KW)
    step, merit, rows = oracle_callables(c["p"], opt=opt)
    n_rows = c["n_cons"] - c["n_dyn"]
    return minimize_loop(step, merit, rows, c["Z"], np.zeros(c["n_cons"]), A.full(c["n_dyn"], np.full(n_rows, A.RHO)), c["n_dyn"], opt, outer, trials)


@functools.lru_cache(maxsize=None)
def oracle_box_run(name="scaled_12x9+con", width=0.3, trials=10):
    """the README's loop in a box (test_gpu_newton_box.oracle_trust_region_run's problem and box) through minimize_loop; returns the
    run, the same loop by newton_box_cases.trust_region_loop, and the box"""
    c = R.case(name)
    p, mu = c["p"], c["mu"]
    step0, merit, rows = oracle_callables(p)
    phi0, Z0 = merit(c["Z"], mu, None)
    lo, hi = B.loop_box(Z0, c["ref"]["C"], width)
    step, merit, rows = oracle_callables(p, lo, hi)
    run = minimize_loop(step, merit, rows, Z0, mu, None, c["n_dyn"], None, 1, trials)

    def old_step(Z, delta):
        info, Zp, _ = step(Z, delta, mu, None)
        return info[6], int(info[0]), Zp

    old = B.trust_region_loop(old_step, lambda Zp: merit(Zp, mu, None), Z0, phi0, trials=trials)
    return run, old, (lo, hi)
