"""High-precision reference for one interval of a TimeDependentBilinearIntegrator (TEST INFRASTRUCTURE ONLY): the DISCRETE map, values
only, in the exact-integer fixed point of tests/hp_reference.py (units of 2^-320; `fx`, `to_float`, `mul`, `scale` are that module's).

The ODE of the reference project's integrator, on the normalised interval tau in [0, 1]:

    dx / dtau = dt_k G(u(tau), t_k + tau dt_k) x,   G(u, t) = sum_{j=0..m} ubar_j (G_j + sum_c phi_c(t) H_cj),  ubar_0 = 1,
    phi_c = cos(omega_c t) | sin(omega_c t),   u(tau) = u_k (order 0)  or  u_k + tau (u_{k+1} - u_k) (order 1),

advanced by the classical Runge-Kutta scheme of the textbook tableau (c = 0, 1/2, 1/2, 1; b = 1/6, 1/3, 1/3, 1/6) on S steps of
h = 1 / S.  h never appears as a number: a stage time is the rational a / (2 S), a = 0 .. 2 S, and h / 2, h and h / 6 are divisions
by 2 S, S and 6 S, each rounded to nearest at 2^-320.  `flow` is the only statement of the scheme in this file; it propagates a
matrix of columns.  There is no variational recursion, no discrete adjoint and no table of derivative jets here: every derivative
is a central difference of `flow` in fixed point --

    first derivatives in theta = (u_k, t_k, dt_k, u_{k+1}):   (f(+h) - f(-h)) / 2h              at h = 2^-80
        truncation h^2 f''' / 6 ~ 2^-160 |f'''|, rounding 2^-320 2^79 (steps x stages x n) ~ 2^-225
    second derivatives of mu' flow x in (theta, theta):       (f(+h) - 2 f + f(-h)) / h^2  and
                                                              (f(++) - f(+-) - f(-+) + f(--)) / 4h^2   at h = 2^-64
        truncation h^2 f'''' / 12 ~ 2^-131 |f''''|, rounding 4 2^-320 2^128 (steps x stages x n) ~ 2^-175
        (|f''''| stays far below 2^30 at ||dt G|| <= 3, |omega| <= 1.7: both estimates sit below 2^-100)
    the (x, theta) block:  d/d theta of mu' flow e_i, the first difference above of the propagated unit vector e_i

and the (x, x) block is zero, the map being linear in x.  sin and cos are their Taylor series on the exact fixed-point argument
(|omega t| <= 8 in the tests: the largest term is 8^8 / 8! = 416, nothing at 320 bits).
"""
import numpy as np

import hp_reference as HP
from hp_reference import FRAC_BITS, fx, mul, to_float  # noqa: F401  (re-exported for the cases module)

ONE = HP.ONE
HALF = HP.HALF
DIFF_BITS = 80            # first central differences
DIFF2_BITS = 64           # second central differences


def rdiv(a, d):
    """a / d for an int or object array a and a positive int d, rounded to nearest."""
    return (a + (d >> 1)) // d


def smul(a, b):
    """Fixed-point product of two scalars."""
    return (int(a) * int(b) + HALF) >> FRAC_BITS


def sincos(a):
    """(sin a, cos a) of the fixed-point scalar a: the Taylor series, term by term until a term vanishes at 2^-320."""
    a = int(a)
    s, c, term, k = 0, 0, ONE, 0
    while term != 0:
        sign = -1 if (k >> 1) & 1 else 1
        if k & 1:
            s += sign * term
        else:
            c += sign * term
        k += 1
        term = rdiv(smul(term, a), k)
    return s, c


def family(G, mods):
    """(B, kinds, omegas) in fixed point: B[0] = G (m + 1, n, n), B[1 + c] = H_c; kinds[c] "cos" | "sin", omegas[c]."""
    B = [fx(G)] + [fx(H) for _, _, H in mods]
    return B, [k for k, _, _ in mods], [int(fx(w)) for _, w, _ in mods]


def generator(fam, order, a, den, uk, uk1, tk, dt):
    """dt G(u(tau), t_k + tau dt) at tau = a / den, fixed point (n, n)."""
    B, kinds, omegas = fam
    t = tk + rdiv(dt * a, den)
    u = [int(p) + rdiv((int(q) - int(p)) * a, den) for p, q in zip(uk, uk1)] if order == 1 else [int(p) for p in uk]
    ubar = [ONE] + u
    phi = [ONE]
    for kind, w in zip(kinds, omegas):
        s, c = sincos(smul(w, t))
        phi.append(c if kind == "cos" else s)
    acc = None
    for c, Bc in enumerate(B):
        for j, uj in enumerate(ubar):
            term = Bc[j] * smul(smul(phi[c], uj), dt)
            acc = term if acc is None else acc + term
    return (acc + HALF) >> FRAC_BITS


def flow(fam, order, S, uk, uk1, tk, dt, Y):
    """The discrete map applied to the columns Y (n, c): S classical Runge-Kutta steps of h = 1 / S."""
    Y = Y + 0
    M_next = generator(fam, order, 0, 2 * S, uk, uk1, tk, dt)
    for i in range(S):
        M1 = M_next
        M2 = generator(fam, order, 2 * i + 1, 2 * S, uk, uk1, tk, dt)
        M_next = M4 = generator(fam, order, 2 * i + 2, 2 * S, uk, uk1, tk, dt)
        k1 = mul(M1, Y)
        k2 = mul(M2, Y + rdiv(k1, 2 * S))
        k3 = mul(M2, Y + rdiv(k2, 2 * S))
        k4 = mul(M4, Y + rdiv(k3, S))
        Y = Y + rdiv(k1 + 2 * k2 + 2 * k3 + k4, 6 * S)
    return Y


def _pack(uk, tk, dt, uk1, order):
    return [int(v) for v in uk] + [int(tk), int(dt)] + ([int(v) for v in uk1] if order == 1 else [])


def _unpack(th, m, order):
    return th[:m], (th[m + 2:] if order == 1 else th[:m]), th[m], th[m + 1]


def _dot(a, b):
    return (int(np.sum(a * b)) + HALF) >> FRAC_BITS


def interval(G, mods, order, S, X, uk, tk, dt, uk1, MU=None, cols=(), extra=None):
    """One interval at theta = (uk, tk, dt, uk1) (float64; uk1 ignored at order 0) for the states X (n, P): P members driven by
    the same system, one column each, MU (n, P) their multipliers or None, `cols` the x indices whose Phi columns are wanted, `extra`
    (n, e) float64 further columns to propagate.  Returns FIXED-POINT arrays:
      y (n, P) = Phi x,  Phi_cols (n, len(cols)),  extra (n, e) = Phi extra,
      dth [p] of (n, P): d (Phi x) / d theta_b,  p = m + 2 (+ m at order 1), theta in the order (u_k, t_k, dt_k, u_{k+1}),
      and with MU:  Hxth (P, len(cols), p) = d (mu' Phi e_i) / d theta_b,  Hthth (P, p, p) = d^2 (mu' Phi x) / d theta_a d theta_b.
    Signs are those of the map; the defect x_{k+1} - Phi x takes the opposite ones (tests/tdbhp_cases.py)."""
    fam = family(G, mods)
    n = fam[0][0].shape[1]
    m = len(uk)
    X = fx(np.asarray(X, dtype=np.float64).reshape(n, -1))
    P = X.shape[1]
    th0 = _pack(fx(uk), int(fx(tk)), int(fx(dt)), fx(uk1) if order == 1 else [], order)
    p = len(th0)
    E = HP.unit_columns(n, cols)
    parts = [X, E] + ([fx(np.asarray(extra, dtype=np.float64).reshape(n, -1))] if extra is not None else [])

    def run(th, Y):
        a, b, t, d = _unpack(th, m, order)
        return flow(fam, order, S, a, b, t, d, Y)

    base = run(th0, np.concatenate(parts, axis=1))
    out = dict(y=base[:, :P], Phi_cols=base[:, P:P + len(cols)], extra=base[:, P + len(cols):], p=p)
    MUf = None if MU is None else fx(np.asarray(MU, dtype=np.float64).reshape(n, -1))
    Y1 = np.concatenate([X, E], axis=1) if MUf is not None else X
    h = 1 << (FRAC_BITS - DIFF_BITS)
    out["dth"] = []
    Hxth = HP.zeros((P, len(cols), p))
    for b in range(p):
        tp, tm = list(th0), list(th0)
        tp[b] += h
        tm[b] -= h
        D = (run(tp, Y1) - run(tm, Y1)) << (DIFF_BITS - 1)
        out["dth"].append(D[:, :P])
        if MUf is not None:
            for q in range(P):
                Hxth[q, :, b] = (mul(MUf[:, q], D[:, P:]))
    if MUf is None:
        return out
    out["Hxth"] = Hxth
    h2 = 1 << (FRAC_BITS - DIFF2_BITS)

    def f(shift):
        th = list(th0)
        for b, s in shift:
            th[b] += s * h2
        Y = run(th, X)
        return [_dot(MUf[:, q], Y[:, q]) for q in range(P)]

    f0 = [_dot(MUf[:, q], out["y"][:, q]) for q in range(P)]
    Hthth = HP.zeros((P, p, p))
    for a in range(p):
        fp, fm = f([(a, 1)]), f([(a, -1)])
        for q in range(P):
            Hthth[q, a, a] = (fp[q] - 2 * f0[q] + fm[q]) << (2 * DIFF2_BITS)
        for b in range(a):
            v = [f([(a, sa), (b, sb)]) for sa, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
            for q in range(P):
                Hthth[q, a, b] = Hthth[q, b, a] = (v[0][q] - v[1][q] - v[2][q] + v[3][q]) << (2 * DIFF2_BITS - 2)
    out["Hthth"] = Hthth
    return out
