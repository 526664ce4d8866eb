"""High-precision reference for one interval of a BilinearIntegrator (TEST INFRASTRUCTURE ONLY).

Exact-integer fixed point: a number is a Python int counting units of 2^-320, a matrix a numpy object array of such ints.  At
320 bits the hump of a Taylor series of exp(M) with ||M|| = 20 (e^20, 29 bits) is of no concern, so the series is summed as it
stands: the matrix exponential with heavy scaling (||M / 2^s||_1 <= 2^-8) and s squarings, the action exp(M) v with no scaling at
all.  Nothing here plans anything, and nothing is shared with the codes under test: no SciPy expm / expm_frechet, none of the
oracle's block functions, no second-derivative formula (second derivatives are central differences of the first derivatives at a
step of 2^-80: truncation ~ 2^-160, rounding ~ 2^-240).

For A = dt (G_0 + sum_j u_j G_j) and the defect  x_next - exp(A) x  of bilinear_integrator.jl:81, `interval` returns
    E = exp(A),  the defect,  the u_j columns L(A, dt G_j) x  (top half of exp([[A, dt G_j], [0, A]]) [0; x]),
    the dt column G(u) E x,  and -- for a multiplier mu -- the Hessian of mu'(defect) in (x, u, dt),
with the signs of the quantities themselves; `tests/hp_cases.py` places them with the defect's signs.
"""
import numpy as np

FRAC_BITS = 320
ONE = 1 << FRAC_BITS
HALF = ONE >> 1
DIFF_BITS = 80           # central-difference step 2^-80


def fx(a):
    """float64 array -> fixed point, exactly (a double is an integer times a power of two no smaller than 2^-1074; what lies
    below 2^-320 is floored away, which no input of the tests has)."""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for idx, v in np.ndenumerate(a):
        num, den = float(v).as_integer_ratio()
        out[idx] = (num << FRAC_BITS) // den
    return out


def to_float(a):
    """fixed point -> float64, correctly rounded (int / int is correctly rounded in Python)."""
    a = np.asarray(a, dtype=object)
    out = np.empty(a.shape, dtype=np.float64)
    for idx, v in np.ndenumerate(a):
        out[idx] = int(v) / ONE
    return out


def mul(A, B):
    """Fixed-point product of two arrays (matrix product for 2-D operands, as numpy's dot), rounded to nearest."""
    return (np.dot(A, B) + HALF) >> FRAC_BITS


def scale(s, A):
    """Fixed-point scalar s times array A."""
    return (A * int(s) + HALF) >> FRAC_BITS


def eye(n):
    out = np.zeros((n, n), dtype=object)
    for i in range(n):
        out[i, i] = ONE
    return out + 0 * ONE          # every entry a Python int


def zeros(shape):
    out = np.empty(shape, dtype=object)
    out.fill(0)
    return out


def norm1(M):
    """max column sum of |M|, as a fixed-point int."""
    return max(int(sum(abs(int(v)) for v in M[:, j])) for j in range(M.shape[1]))


def _is_zero(T):
    return all(int(v) == 0 for v in T.flat)


def expm(M):
    """exp(M) of a square fixed-point matrix: Taylor series of M / 2^s with ||M / 2^s||_1 <= 2^-8, summed until a term vanishes
    at 2^-320, then s squarings."""
    n = M.shape[0]
    s = max(0, norm1(M).bit_length() - FRAC_BITS + 8)
    X = (M + ((1 << s) >> 1)) >> s
    T = eye(n)
    term = eye(n)
    k = 0
    while not _is_zero(term):
        k += 1
        term = (mul(term, X) + (k >> 1)) // k
        T = T + term
    for _ in range(s):
        T = mul(T, T)
    return T


def expm_action(M, V):
    """exp(M) V for a fixed-point vector or matrix of columns V: the Taylor series as it stands, no scaling."""
    acc = V + 0
    term = V + 0
    k = 0
    while not _is_zero(term):
        k += 1
        term = (mul(M, term) + (k >> 1)) // k
        acc = acc + term
    return acc


def frechet_action(A, B, X):
    """(L(A, B) X, exp(A) X) as the two halves of exp([[A, B], [0, A]]) [0; X]."""
    n = A.shape[0]
    M = zeros((2 * n, 2 * n))
    M[:n, :n] = A
    M[:n, n:] = B
    M[n:, n:] = A
    X = X.reshape(n, -1)
    V = np.concatenate([zeros(X.shape), X], axis=0)
    R = expm_action(M, V)
    return R[:n], R[n:]


def _dot(a, b):
    """Fixed-point sum of products over every entry."""
    return (int(np.sum(a * b)) + HALF) >> FRAC_BITS


def _first_order(Gf, X, u, dt, MU=None):
    """Everything of first order at (u, dt), in fixed point.  Gf (m+1, n, n), X (n, c) columns the generators act on alike
    (c = 1 for a plain integrator), u (m,), dt: fixed point.  MU (n, c) or None."""
    m = Gf.shape[0] - 1
    Gu = Gf[0] + 0
    for j in range(m):
        Gu = Gu + scale(u[j], Gf[1 + j])
    A = scale(dt, Gu)
    LX, EX = [], None
    for j in range(m):
        top, EX = frechet_action(A, scale(dt, Gf[1 + j]), X)
        LX.append(top)
    if EX is None:
        EX = expm_action(A, X)
    GEX = mul(Gu, EX)
    out = dict(A=A, EX=EX, LX=LX, GEX=GEX)
    if MU is not None:
        # gradient of mu'(x_next - exp(A) x) in (x, u, dt)
        out["gx"] = -expm_action(A.T.copy(), MU)
        out["gu"] = [-_dot(MU, L) for L in LX]
        out["gdt"] = -_dot(MU, GEX)
    return out


def unit_columns(n, cols):
    """The unit vectors e_c, c in cols, as the columns of an (n, len(cols)) fixed-point matrix."""
    V = zeros((n, len(cols)))
    for j, c in enumerate(cols):
        V[int(c), j] = ONE
    return V


def interval(G, x, u, dt, x_next, mu=None, want_E=True, E_cols=None):
    """One interval.  G (m+1, n, n) float64; x, x_next, mu: (n,) or, for generators I_c (x) G acting on c segments alike, (n, c)
    columns; u (m,), dt: float64.  Returns a dict of FIXED-POINT arrays (round with `to_float`):
      A, E (n, n; None unless want_E), EX = exp(A) x, defect = x_next - EX, LX [m] of (n, c), GEX (n, c),
      with E_cols (a sequence of column indices): E_cols = E[:, E_cols], as the action of exp(A) on those unit vectors -- no
      exponential is formed for them, so sampled columns of a large E stay affordable (want_E=False),
      and with mu: H, the (nx + m + 1)^2 Hessian of mu'(defect) in (x, u, dt), x column-major over (n, c) flattened as
      segment-major (column c0 of X first) -- its (x, x) block is zero, the defect being linear in x.
    """
    Gf = fx(G)
    X = fx(np.asarray(x, dtype=np.float64).reshape(Gf.shape[1], -1))
    Xn = fx(np.asarray(x_next, dtype=np.float64).reshape(Gf.shape[1], -1))
    uf, dtf = fx(u), int(fx(dt))
    m = Gf.shape[0] - 1
    MU = None if mu is None else fx(np.asarray(mu, dtype=np.float64).reshape(Gf.shape[1], -1))
    base = _first_order(Gf, X, uf, dtf, MU)
    out = dict(A=base["A"], EX=base["EX"], LX=base["LX"], GEX=base["GEX"], defect=Xn - base["EX"],
               E=expm(base["A"]) if want_E else None)
    if E_cols is not None:
        out["E_cols"] = expm_action(base["A"], unit_columns(Gf.shape[1], E_cols))
    if MU is None:
        return out
    nx = X.size
    h = 1 << (FRAC_BITS - DIFF_BITS)
    cols = []
    for d in range(m + 1):
        def at(sign):
            uu = uf.copy()
            dd = dtf
            if d < m:
                uu[d] = int(uu[d]) + sign * h
            else:
                dd = dd + sign * h
            return _first_order(Gf, X, uu, dd, MU)
        p, q = at(+1), at(-1)
        # (g(+h) - g(-h)) / (2 h), h = 2^-80: a shift by 79 bits
        col = [(a - b) << (DIFF_BITS - 1) for a, b in zip(p["gx"].T.reshape(-1), q["gx"].T.reshape(-1))]
        col += [(a - b) << (DIFF_BITS - 1) for a, b in zip(p["gu"], q["gu"])]
        col.append((p["gdt"] - q["gdt"]) << (DIFF_BITS - 1))
        cols.append(col)
    H = zeros((nx + m + 1, nx + m + 1))
    for d in range(m + 1):
        for r in range(nx + m + 1):
            H[r, nx + d] = cols[d][r]
    for d in range(m + 1):          # the x rows of the (u, dt) columns, mirrored; (u, dt) x (u, dt) averaged over both orders
        for r in range(nx):
            H[nx + d, r] = H[r, nx + d]
        for e in range(d):
            v = (int(H[nx + e, nx + d]) + int(H[nx + d, nx + e])) >> 1
            H[nx + e, nx + d] = H[nx + d, nx + e] = v
    out["H"] = H
    out["gx"], out["gu"], out["gdt"] = base["gx"], base["gu"], base["gdt"]
    return out
