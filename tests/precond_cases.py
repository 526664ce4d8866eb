"""Shared by the tests of the L-BFGS-preconditioned truncated-Newton step (test_precond_plan_header.py, test_precond_reference.py,
test_gpu_precond.py): csrc/dto_precond_plan.h restated in NumPy -- the Gram entries, admission, the compact application and the loop
around ANY product -- and the textbook two-loop recursion the application is judged by.

The dot, the decision and the box rules are imported (test_gpu_newton_step.dot, newton_box_cases), not copied."""
import math

import numpy as np

import newton_box_cases as B
from newton_box_cases import CONTINUE, CONVERGED, FREE, HIT_LO, MAX_ITER, NOT_FINITE
from test_gpu_newton_step import dot

EPS = 2.0 ** -26          # PRECOND_EPS
MAX_PAIRS = 16


# ------------------------------------------------------------------------------------------------------------ the store
class Store:
    """the pair store's bookkeeping: capacity m, the pairs oldest first"""

    def __init__(self, m):
        self.m, self.S, self.Y = m, [], []

    def push(self, s, y):
        self.S.append(np.array(s, dtype=np.float64))
        self.Y.append(np.array(y, dtype=np.float64))
        if len(self.S) > self.m:
            del self.S[0], self.Y[0]

    def harvested(self, pairs):
        """what a call that took `pairs` (oldest first) leaves: the last m of them, or the store as it was without one"""
        if pairs:
            self.S, self.Y = [np.array(d) for d, _ in pairs[-self.m:]], [np.array(w) for _, w in pairs[-self.m:]]

    @property
    def count(self):
        return len(self.S)


# --------------------------------------------------------------------------------------------------- preparation, application
def prepare_restated(S, Y, F0, dot=dot):
    """Gram entries over F0 in the dot's order, admission oldest to newest, gamma, R and M over the admitted pairs"""
    cnt = len(S)
    Sm, Ym = [np.where(F0, s, 0.0) for s in S], [np.where(F0, y, 0.0) for y in Y]
    SY, YY = np.zeros((cnt, cnt)), np.zeros((cnt, cnt))
    for j in range(cnt):
        for i in range(j + 1):
            SY[i, j] = dot(Sm[i], Ym[j])
            YY[i, j] = YY[j, i] = dot(Ym[i], Ym[j])
    SS = [dot(s, s) for s in Sm]
    with np.errstate(all="ignore"):
        idx = [k for k in range(cnt) if math.isfinite(SY[k, k]) and math.isfinite(SS[k]) and math.isfinite(YY[k, k])
               and SY[k, k] > EPS * np.sqrt(np.float64(SS[k]) * np.float64(YY[k, k]))]
    q = len(idx)
    gamma = float(np.float64(SY[idx[-1], idx[-1]]) / np.float64(YY[idx[-1], idx[-1]])) if q else 1.0
    Rm, M = np.zeros((q, q)), np.zeros((q, q))
    for a in range(q):
        for b in range(q):
            if a <= b:
                Rm[a, b] = SY[idx[a], idx[b]]
            M[a, b] = gamma * YY[idx[a], idx[b]]
            if a == b:
                M[a, b] = SY[idx[a], idx[a]] + M[a, b]
    return dict(idx=idx, gamma=gamma, R=Rm, M=M, S=S, Y=Y)


def coeffs_restated(P, u, v):
    """the two triangular solves, every operation on its own in the header's order"""
    q, R, M, gamma = len(P["idx"]), P["R"], P["M"], np.float64(P["gamma"])
    a, c1 = np.zeros(q), np.zeros(q)
    with np.errstate(all="ignore"):
        for i in range(q - 1, -1, -1):
            t = np.float64(u[i])
            for k in range(i + 1, q):
                t = t - R[i, k] * a[k]
            a[i] = t / R[i, i]
        for i in range(q):
            acc = np.float64(0.0)
            for k in range(q):
                acc = acc + M[i, k] * a[k]
            t = acc - gamma * np.float64(v[i])
            for k in range(i):
                t = t - R[k, i] * c1[k]
            c1[i] = t / R[i, i]
    return c1, -a


def apply_restated(P, r, F, on=True, dot=dot):
    """(z, r . z over F): z = P_F H P_F r, or r on F without an admitted pair or with the preconditioner off"""
    rf = np.where(F, r, 0.0)
    idx = P["idx"]
    if not (on and idx):
        return rf, dot(rf, rf)
    u = [dot(np.where(F, P["S"][k], 0.0), rf) for k in idx]
    v = [dot(np.where(F, P["Y"][k], 0.0), rf) for k in idx]
    c1, c2 = coeffs_restated(P, u, v)
    gamma = P["gamma"]
    a1, a2 = np.zeros(r.size), np.zeros(r.size)
    with np.errstate(all="ignore"):
        for e, k in enumerate(idx):
            a1 = a1 + c1[e] * P["S"][k]
            a2 = a2 + c2[e] * P["Y"][k]
        z = np.where(F, (gamma * r + a1) + gamma * a2, 0.0)
    return z, dot(rf, z)


def precondition_restated(S, Y, R, nonfixed):
    """dto_newton_precondition: F0 = F = nonfixed; R (n_cols, n) or (n,)"""
    P = prepare_restated(S, Y, nonfixed)
    R = np.asarray(R, dtype=np.float64)
    if R.ndim == 1:
        return apply_restated(P, R, nonfixed)[0]
    return np.array([apply_restated(P, r, nonfixed)[0] for r in R])


def rz_bad(rz):
    return not (math.isfinite(rz) and rz > 0.0)


# ---------------------------------------------------------------------------------------------------------------- the loop
def precond_loop(product, g, nonfixed, Z, S=(), Y=(), lo=None, hi=None, radius=0.0, shift=0.0, rtol=1e-6, atol=0.0, max_iter=50, harvest=False,
                 dot=dot):
    """newton_box_cases.box_loop with dto_precond_plan.h's changes.  Returns a dict: p, info [16], trace [iterations][8], states, Zp, and
    pairs: the (d, w) the harvest took, oldest first."""
    n = Z.size
    lo = np.full(n, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(n, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    state = B.classify_restated(Z, lo, hi, g, nonfixed)
    F0 = state == FREE
    g0 = np.where(F0, g, 0.0)
    r, x = g0.copy(), np.zeros(n)
    held = int(np.sum((state == B.HELD_LO) | (state == B.HELD_HI)))
    rr0 = rr_new = dot(r, r)
    P = prepare_restated(list(S), list(Y), F0, dot)
    on = len(P["idx"]) > 0
    z, rz = apply_restated(P, r, F0, on, dot)
    status, j, hits, restarts, kappa, dd, fallbacks = (CONVERGED if rr0 == 0.0 else CONTINUE), 0, 0, 0, 0.0, 0.0, 0
    if status == CONTINUE and on and rz_bad(rz):
        on, fallbacks, rz = False, 1, rr0
    rz0 = rz
    d = -(r if fallbacks else z)
    trace, pairs = [], []
    while status == CONTINUE and j < max_iter:
        j += 1
        y = product(d)
        with np.errstate(all="ignore"):
            w = np.where(F0, y + shift * d, 0.0)
        t = B.breakpoints_restated(Z, x, d, lo, hi, state == FREE)
        tau_box = B.min_restated(t)
        kappa, dd, pd, pp = dot(d, w), dot(d, d), dot(x, d), dot(x, x)
        status, s = B.box_decide_restated(kappa, dd, pd, pp, rz, radius, tau_box, j)
        if harvest and math.isfinite(kappa) and kappa > 0.0:
            pairs.append((d.copy(), w.copy()))
        n_hit = 0
        if status != NOT_FINITE:
            with np.errstate(all="ignore"):
                x = x + s * d
                r = r + s * w
            x, state, n_hit = B.clamp_restated(Z, x, d, lo, hi, t, s, state)
        F = state == FREE
        rf = np.where(F, r, 0.0)
        rr_new = dot(rf, rf)
        hits += n_hit
        z, rz_new = apply_restated(P, r, F, on, dot)
        if status == CONTINUE and np.sqrt(rr_new) <= max(atol, rtol * np.sqrt(rr0)):
            status = CONVERGED
        fallback = status == CONTINUE and on and rz_bad(rz_new)
        if fallback:
            on, fallbacks = False, fallbacks + 1
        trace.append([kappa, dd, s, rr_new, tau_box, float(n_hit), rz_new, 1.0 if on else 0.0])
        if status != CONTINUE:
            break
        rz_use = rr_new if fallback else rz_new
        xdir = r if fallback else z
        if n_hit > 0 or fallback:
            d = np.where(F, -xdir, 0.0)
            restarts += 1 if n_hit > 0 else 0
        else:
            with np.errstate(all="ignore"):
                d = np.where(state >= HIT_LO, 0.0, (np.float64(rz_use) / np.float64(rz)) * d - xdir)
        rz = rz_use
        if j == max_iter:
            status = MAX_ITER
    pg, pr, pp = dot(x, g0), dot(x, r), dot(x, x)
    with np.errstate(all="ignore"):
        curvature = float(np.float64(kappa) / np.float64(dd)) if j >= 1 else 0.0
        info = np.array([status, j, np.sqrt(rr0), np.sqrt(rr_new), np.sqrt(pp), pg, -0.5 * (pg + pr), curvature, held, hits, restarts,
                         int(np.sum(state == FREE)), len(P["idx"]), len(pairs), fallbacks, np.sqrt(np.float64(rz0))], dtype=np.float64)
    Zp = np.where(state == B.HIT_LO, lo, np.where(state == B.HIT_HI, hi, Z + x))
    return dict(p=x, info=info, trace=np.array(trace).reshape(len(trace), 8), states=state.astype(np.float64), Zp=Zp, pairs=pairs)


# ------------------------------------------------------------------------------------------------- the textbook reference
def two_loop(S, Y, r, dtype=np.float64):
    """Nocedal's two-loop recursion for the BFGS inverse with H0 = (s_k . y_k / y_k . y_k) I of the newest pair, in `dtype`"""
    S, Y = [np.asarray(s, dtype=dtype) for s in S], [np.asarray(y, dtype=dtype) for y in Y]
    q = np.asarray(r, dtype=dtype).copy()
    rho = [dtype(1) / (s @ y) for s, y in zip(S, Y)]
    alpha = [None] * len(S)
    for k in range(len(S) - 1, -1, -1):
        alpha[k] = rho[k] * (S[k] @ q)
        q = q - alpha[k] * Y[k]
    if S:
        q = ((S[-1] @ Y[-1]) / (Y[-1] @ Y[-1])) * q
    for k in range(len(S)):
        beta = rho[k] * (Y[k] @ q)
        q = q + (alpha[k] - beta) * S[k]
    return q
