"""Shared by the tests of the bound-constrained truncated-Newton step (test_newton_box_plan_header.py, test_newton_box_scenarios.py,
test_gpu_newton_box.py): the loop of include/dto_engine.h, "Bound-constrained truncated-Newton step", restated in NumPy around ANY product
(the header's own program, the oracle's dense matrix, the engine's reduced_hessian_product), and the scenarios, which are built from
reduced_cases / long_cases and the ORACLE's reduced Hessian and gradient only.

The dot order, the decision and the halving tree are test_newton_plan_header.py's restatements (imported, not copied); the vectorised dot
is test_gpu_newton_step.py's."""
import functools
import math

import numpy as np

import long_cases as LC
import reduced_cases as R
from test_gpu_newton_step import dot
from test_newton_plan_header import CONTINUE, CONVERGED, MAX_ITER, NEG_CURVATURE, NOT_FINITE, decide_restated

FIXED, FREE, HELD_LO, HELD_HI, HIT_LO, HIT_HI = 0, 1, 2, 3, 4, 5
SIGMA = R.SIGMA


# ------------------------------------------------------------------------------------------------------ the rules, restated
def classify_restated(Z, lo, hi, g, nonfixed):
    """the lower bound is tested first; a fixed entry reads nothing"""
    with np.errstate(invalid="ignore"):
        s = np.where((Z <= lo) & (g > 0), HELD_LO, np.where((Z >= hi) & (g < 0), HELD_HI, FREE))
    return np.where(nonfixed, s, FIXED)


def breakpoints_restated(Z, x, d, lo, hi, F):
    """t_i = max(0, (bound_i - (Z_i + x_i)) / d_i) on F with d_i != 0 (a NaN stays a NaN, -0 becomes +0), +inf elsewhere"""
    with np.errstate(all="ignore"):
        q = (np.where(d > 0, hi, lo) - (Z + x)) / d
    t = np.where(np.isnan(q), q, np.where(q > 0, q, 0.0))
    return np.where(F & ((d > 0) | (d < 0)), t, np.inf)


def min_restated(t):
    """the smallest entry that is no NaN, +inf without one"""
    return float(np.fmin.reduce(t, initial=np.inf)) if t.size else math.inf


def box_decide_restated(kappa, dd, pd, pp, rr, radius, tau_box, j):
    status, s = decide_restated(kappa, dd, pd, pp, rr, radius, j)
    if status == NOT_FINITE:
        return status, s
    if status == NEG_CURVATURE and radius == 0 and math.isfinite(tau_box):
        return CONTINUE, tau_box
    if s > tau_box:
        return CONTINUE, tau_box
    return status, s


def clamp_restated(Z, x, d, lo, hi, t, s, state):
    """behind x = x + s d: the free entries that reached a bound, set onto it; returns (x, state, n_hit)"""
    F = state == FREE
    with np.errstate(invalid="ignore"):
        up = F & (d > 0) & ((t <= s) | (Z + x >= hi))
        dn = F & (d < 0) & ((t <= s) | (Z + x <= lo))
    x = np.where(up, hi - Z, np.where(dn, lo - Z, x))
    return x, np.where(up, HIT_HI, np.where(dn, HIT_LO, state)), int(np.sum(up) + np.sum(dn))


def box_loop(product, g, nonfixed, Z, lo=None, hi=None, radius=0.0, shift=0.0, rtol=1e-6, atol=0.0, max_iter=50, dot=dot):
    """The loop.  product(d) -> y = T'HT d; g the reduced gradient; nonfixed: the entries that are neither dependent nor masked.
    Returns a dict: p, info [12], trace [iterations][6], states, Zp, and per iteration the iterate (xs) and the two smallest
    breakpoints (gaps), which the scenario tests judge."""
    n = Z.size
    lo = np.full(n, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(n, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    state = classify_restated(Z, lo, hi, g, nonfixed)
    F0 = state == FREE
    g0 = np.where(F0, g, 0.0)
    r, x, d = g0.copy(), np.zeros(n), -g0
    held = int(np.sum((state == HELD_LO) | (state == HELD_HI)))
    rr0 = rr = rr_new = dot(r, r)
    status, j, hits, restarts, kappa, dd = (CONVERGED if rr0 == 0.0 else CONTINUE), 0, 0, 0, 0.0, 0.0
    trace, xs, gaps = [], [], []
    while status == CONTINUE and j < max_iter:
        j += 1
        y = product(d)
        with np.errstate(all="ignore"):
            w = np.where(F0, y + shift * d, 0.0)
        t = breakpoints_restated(Z, x, d, lo, hi, state == FREE)
        tau_box = min_restated(t)
        finite = np.sort(t[np.isfinite(t)])
        gaps.append((finite[0] if finite.size else math.inf, finite[1] if finite.size > 1 else math.inf))
        kappa, dd, pd, pp = dot(d, w), dot(d, d), dot(x, d), dot(x, x)
        status, s = box_decide_restated(kappa, dd, pd, pp, rr, radius, tau_box, j)
        n_hit = 0
        if status != NOT_FINITE:
            with np.errstate(all="ignore"):
                x = x + s * d
                r = r + s * w
            x, state, n_hit = clamp_restated(Z, x, d, lo, hi, t, s, state)
        F = state == FREE
        rf = np.where(F, r, 0.0)
        rr_new = dot(rf, rf)
        hits += n_hit
        trace.append([kappa, dd, s, rr_new, tau_box, float(n_hit)])
        xs.append(x.copy())
        if status == CONTINUE and np.sqrt(rr_new) <= max(atol, rtol * np.sqrt(rr0)):
            status = CONVERGED
        if status != CONTINUE:
            break
        if n_hit > 0:
            d = np.where(F, -r, 0.0)
            restarts += 1
        else:
            d = np.where(state >= HIT_LO, 0.0, (rr_new / rr) * d - r)
        rr = rr_new
        if j == max_iter:
            status = MAX_ITER
    pg, pr, pp = dot(x, g0), dot(x, r), dot(x, x)
    with np.errstate(all="ignore"):
        curvature = float(np.float64(kappa) / np.float64(dd)) if j >= 1 else 0.0
    info = np.array([status, j, np.sqrt(rr0), np.sqrt(rr_new), np.sqrt(pp), pg, -0.5 * (pg + pr), curvature, held, hits, restarts,
                     int(np.sum(state == FREE))], dtype=np.float64)
    Zp = np.where(state == HIT_LO, lo, np.where(state == HIT_HI, hi, Z + x))
    return dict(p=x, info=info, trace=np.array(trace).reshape(len(trace), 6), states=state.astype(np.float64), Zp=Zp, xs=xs, gaps=gaps)


# ---------------------------------------------------------------------------------------------------------- the scenarios
SCENARIOS = ("inf", "half_box", "held", "indefinite_box", "indefinite_box_radius")
CONVEX = ("half_box", "held")


def scenarios_from(Z, C, gC, shift, pstar):
    """(a) .. (e) as keyword sets of the step: Z the point, C the independent entries, gC the reduced gradient on C, shift the convex
    scenarios' shift, pstar the unbounded solution on C.  Bounds that no scenario sets are infinite."""
    n = Z.size

    def box():
        return np.full(n, -np.inf), np.full(n, np.inf)

    out = {"inf": dict(shift=shift, rtol=1e-8, max_iter=40)}
    lo, hi = box()
    order = np.argsort(pstar)
    up, dn = order[::-1][:5], order[:5]
    assert np.all(pstar[up] > 0) and np.all(pstar[dn] < 0)
    hi[C[up]] = Z[C[up]] + 0.5 * pstar[up]
    lo[C[dn]] = Z[C[dn]] + 0.5 * pstar[dn]
    out["half_box"] = dict(lo=lo, hi=hi, shift=shift, rtol=1e-8, max_iter=60)
    # held: the six entries with the largest |g|; four on a bound with -g pointing out of the box, two on a bound with -g pointing in
    lo, hi = box()
    six = np.argsort(-np.abs(gC))[:6]
    for a, i in enumerate(six):
        on_lower = (gC[i] > 0) == (a < 4)
        (lo if on_lower else hi)[C[i]] = Z[C[i]]
    out["held"] = dict(lo=lo, hi=hi, shift=shift, rtol=1e-8, max_iter=60)
    out["held_entries"] = (C[six[:4]], C[six[4:]])
    lo, hi = box()
    lo[C], hi[C] = Z[C] - 1.0, Z[C] + 1.0
    out["indefinite_box"] = dict(lo=lo, hi=hi, shift=0.0, radius=0.0, rtol=1e-8, max_iter=60)
    out["indefinite_box_radius"] = dict(lo=lo, hi=hi, shift=0.0, radius=2.0, rtol=1e-8, max_iter=60)
    for v in out.values():
        if isinstance(v, dict):
            for a in v.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def small_scenarios(name):
    """the scenarios of a case of reduced_cases from the oracle's dense reduced Hessian and gradient:
    shift = 1.5 |lambda_min| + 0.01 lambda_max, p* = solve(Hr + shift I, -g)"""
    c = R.case(name)
    ref, Cidx = c["ref"], c["ref"]["C"]
    Hr = 0.5 * (ref["Hr"] + ref["Hr"].T)
    lam = np.linalg.eigvalsh(Hr)
    shift = 1.5 * abs(lam[0]) + 0.01 * lam[-1]
    gC = ref["r_ref"][Cidx]
    pstar = np.linalg.solve(Hr + shift * np.eye(Cidx.size), -gC)
    return dict(scenarios_from(c["Z"], Cidx, gC, shift, pstar), lam=lam, shift=shift, pstar=pstar)


def oracle_product(name):
    """d -> T'HT d of the oracle's dense matrix, as an n_vars vector"""
    ref = R.case(name)["ref"]
    return lambda d: R.product_ref(ref, d)


@functools.lru_cache(maxsize=None)
def long_scenarios(name):
    """the scenarios of a long case from the oracle's sparse reference (long_cases.case).  No dense matrix exists at this length, so the
    shift is twice the largest |Rayleigh quotient| of eight power iterations with the ORACLE's product (A is then positive definite with
    a condition number of at most 3) and p* comes from forty CG iterations with that product."""
    c = LC.case(name)
    ref, Cidx, Z = c["ref"], c["ref"]["C"], c["Z"]
    prod = lambda v: LC.product_ref(ref, v)
    v = R.free_direction(c["p"], np.random.default_rng(5))
    top = 0.0
    for _ in range(8):
        v = v / np.linalg.norm(v)
        y = prod(v)
        top = max(top, abs(float(v @ y)))
        v = y
    shift = 2.0 * top
    g = np.array(ref["r_ref"])
    x, r = np.zeros(Z.size), g.copy()
    d, rr = -r, float(g @ g)
    for _ in range(40):
        w = prod(d) + shift * d
        w[ref["S"]] = 0.0
        a = rr / float(d @ w)
        x, r = x + a * d, r + a * w
        rr, rr_old = float(r @ r), rr
        d = (rr / rr_old) * d - r
    return dict(scenarios_from(Z, Cidx, g[Cidx], shift, x[Cidx]), shift=shift, pstar=x[Cidx])


def nonfixed_of(p, free=None):
    M = np.ones(p.n_vars, dtype=bool)
    M[R.index_sets(p)[0]] = False
    if free is not None:
        M &= np.asarray(free) != 0.0
    return M


# ------------------------------------------------------------------------------------------------------ the loop of the README
def trust_region_loop(step, merit, Z, phi, trials=10, delta=1.0):
    """The textbook trust-region loop of the README's snippet.  step(Z, delta) -> (predicted, status, Zp); merit(Zp) -> (phi, Zf).
    Returns the accepted iterates, their merit values and per trial whether it was accepted."""
    iterates, values, accepted = [Z], [phi], []
    for _ in range(trials):
        predicted, status, Zp = step(Z, delta)
        phi_t, Z_t = merit(Zp)
        rho = (phi - phi_t) / predicted
        ok = bool(rho > 0.1)
        accepted.append(ok)
        if ok:
            Z, phi = Z_t, phi_t
            iterates.append(Z)
            values.append(phi)
        if rho < 0.25:
            delta /= 4.0
        elif rho > 0.75 and status != CONVERGED:
            delta *= 2.0
    return iterates, values, accepted


def loop_box(Z, C, width):
    """the box of the use test: Z -+ width on the independent entries"""
    lo, hi = np.full(Z.size, -np.inf), np.full(Z.size, np.inf)
    lo[C], hi[C] = Z[C] - width, Z[C] + width
    return lo, hi
