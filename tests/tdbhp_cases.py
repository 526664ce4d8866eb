"""The cases of the time-dependent accuracy tests (tests/test_tdb_hp_reference.py, tests/test_gpu_tdb_accuracy_budget.py): problems
rebuilt from their seeds, the expected callback vectors from tests/tdb_hp_reference.py laid out in the oracle's structure, the metric
of tests/hp_cases.py (the NORMWISE error per interval and quantity class, max|a - b| / max|b| over the class's entries), and the
bars, which a fixture carries with it.

One TimeDependentBilinearIntegrator per problem on the components x[n], u[m], t, dt; N = 4 knots, random generators that are not
skew; t_k = 0.3, 0.9, 1.6, 2.0 and dt_k scaled so that ||dt_k G(u_k, t_k)||_2 is 0.05, 1 and 3 in a shuffled order, so |omega t|
stays below 1.7 (2 + 3 / ||G||) < 8.

Above 64 states (`sample` in CASES) the expected Jacobian holds 16 sampled columns of each Phi block and NaN elsewhere in the block,
as tests/hp_cases.py does with E_k; the (x, theta) entries of the Hessian and the x entries of J' w are known on the same indices.
`*_known` marks what is known; a class is measured over its known entries and every other entry must still be a finite number.

`group` (tdbhp_n72): a second member x_b with its own mu, driven by the same u, t, dt -- the fixture's vectors `*_b` are that
member's, in the layout of the one-member problem; the theta entries of J' w and the (theta, theta) entries of the Hessian, to
which both members add, are stored summed (`JTw_g`, `hess_g`, `JTw_b`, `hess_b`).  `group_problem`, `member_fix` and `member_got`
turn the two-member handle's vectors into two one-member comparisons.

Bars: 16 x the worst error, over the fixture's intervals, of the repository's fp64 restatement of the scheme (tests/tdb_large_cases.py:
step-matrix products and complex steps) against the 320-bit values, floored at hp_cases.BAR_NO_SQUARING = 64 2^-53.  The kernels
sum in other orders than NumPy (MFMA k blocks four deep, lane-split dot products closed by a butterfly) and run the variational
recursion where the yardstick multiplies step matrices: a small multiple; a wrong weight, stage time or term is orders away.  The
generator (tests/golden/make_tdbhp_golden.py) measures the yardstick and writes `classes`, `yard` and `bars` into the fixture;
nothing here reads engine output to set a bar.  The yardstick must stay below hp_cases.ORACLE_CAP = 1e-13 everywhere."""
import hashlib
import os

import numpy as np

import dto_oracle as O
import hp_cases as HC
import hp_reference as HP
import tdb_block_cases as B
import tdb_hp_reference as T
import tdb_large_cases as L

GOLDEN = HC.GOLDEN
N_KNOTS = 4
TIMES = (0.3, 0.9, 1.6, 2.0)
RUNGS = (0.05, 1.0, 3.0)
BAR_FACTOR = 16.0
CASES = {
    "tdbhp_n4": dict(n=4, m=3, order=1, n_mods=2, S=3, seed=1201),       # k_tdb, forward Hessian form
    "tdbhp_n16": dict(n=16, m=3, order=1, n_mods=2, S=4, seed=1202),     # k_tdb, discrete-adjoint Hessian
    "tdbhp_n16_o0": dict(n=16, m=2, order=0, n_mods=0, S=3, seed=1203),  # k_tdb, controls held, no carrier
    "tdbhp_n72": dict(n=72, m=2, order=1, n_mods=2, S=4, seed=1204, sample=16, group=True),   # k_tdb_mfma<32> (n_pad 96)
    "tdbhp_n128": dict(n=128, m=2, order=0, n_mods=1, S=2, seed=1205, sample=16),             # k_tdb_mfma<64>
    "tdbhp_kron": dict(n=36, b=12, r=3, m=2, order=1, n_mods=2, S=2, seed=1206),              # k_tdb_kron, blocks 12 x 3
}
ENGINE_KW = {"tdbhp_kron": dict(block_generators=True)}


def _family(name):
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    if "b" in c:
        return B.kron_family(c["b"], c["r"], c["m"], c["n_mods"], rng)
    n, m = c["n"], c["m"]
    G = rng.standard_normal((m + 1, n, n)) / np.sqrt(n / 4.0)
    mods = [("cos", 1.7, 0.5 * rng.standard_normal((m + 1, n, n)) / np.sqrt(n / 4.0)),
            ("sin", 0.6, 0.5 * rng.standard_normal((m + 1, n, n)) / np.sqrt(n / 4.0))][:c["n_mods"]]
    return G, mods


def problem(name):
    """The case's oracle problem at its seed's point, t_k and the dt ladder set."""
    c = CASES[name]
    G, mods = _family(name)
    p = B.problem_from_family(G, mods, c["m"], c["order"], c["S"], N=N_KNOTS, seed=c["seed"] + 3)
    it = p.integrators[0]
    Zk = p.Z0.reshape(p.N, p.z).copy()
    Zk[:, it.t_off] = TIMES
    perm = np.random.default_rng(c["seed"] + 7).permutation(len(RUNGS))
    for k in range(p.K):
        Gk = it.generator(Zk[k, it.u_off:it.u_off + it.u_dim], Zk[k, it.t_off])
        Zk[k, p.dt_idx] = RUNGS[perm[k]] / np.linalg.norm(Gk, 2)
    Zk[p.K, p.dt_idx] = 0.1
    p.Z0 = Zk.reshape(-1).copy()
    return p


def columns(name):
    """The sampled x indices of a `sample` case (None: all): 0, 15, 16, 31, 32, 63, 64, n - 1 and the rest from the seed."""
    c = CASES[name]
    if "sample" not in c:
        return None
    n = c["n"]
    must = {0, 15, 16, 31, 32, 63, 64, n - 1}
    rest = [int(j) for j in np.random.default_rng(c["seed"] + 29).permutation(n) if int(j) not in must]
    return np.array(sorted(must | set(rest[:c["sample"] - len(must)])), dtype=np.int64)


INPUT_KEYS = ("Z", "mu", "w", "wt", "x_b", "mu_b", "wx_b", "wt_b")


def inputs(name):
    """What a fixture stores that a seed does not give back."""
    p = problem(name)
    c = CASES[name]
    rng = np.random.default_rng(c["seed"] + 13)
    n_cons = c["n"] * p.K
    d = dict(Z=p.Z0.copy(), mu=rng.standard_normal(n_cons), w=rng.standard_normal(p.n_vars), wt=rng.standard_normal(n_cons))
    if c.get("group"):
        d.update(x_b=rng.standard_normal((p.N, c["n"])), mu_b=rng.standard_normal(n_cons), wx_b=rng.standard_normal((p.N, c["n"])),
                 wt_b=rng.standard_normal(n_cons))
    return d


def input_hash(d):
    h = hashlib.sha256()
    for k in INPUT_KEYS:
        if k in d:
            h.update(np.ascontiguousarray(d[k], dtype=np.float64).tobytes())
    return h.hexdigest()


def at_point(name, Z):
    p = problem(name)
    p.Z0 = np.asarray(Z, dtype=np.float64).copy()
    return p, O.OracleEvaluator(p)


def _theta_index(it, z):
    """Columns of theta = (u_k, t_k, dt_k, u_{k+1}) within the two-knot block."""
    idx = [it.u_off + j for j in range(it.u_dim)] + [it.t_off, it.dt_idx]
    if it.spline_order == 1:
        idx += [z + it.u_off + j for j in range(it.u_dim)]
    return idx


def expected(name, d, intervals=None):
    """The expected callback vectors of the case at the inputs d, from tests/tdb_hp_reference.py, rounded to fp64 once.
    `intervals`: compute these alone (the others' entries are left zero; for the regeneration test)."""
    p, ev_o = at_point(name, d["Z"])
    it = p.integrators[0]
    n, m, z, K, N = it.x_dim, it.u_dim, p.z, p.K, p.N
    group = "x_b" in d
    P = 2 if group else 1
    cols = columns(name)
    sampled = cols is not None
    ecols = np.arange(n) if cols is None else cols
    Zk = d["Z"].reshape(N, z)
    xs = slice(it.x_off, it.x_off + n)
    Xs = [Zk[:, xs]] + ([d["x_b"]] if group else [])
    MUs = [d["mu"].reshape(K, n)] + ([d["mu_b"].reshape(K, n)] if group else [])
    W = d["w"].reshape(N, z)
    WXs = [W[:, xs]] + ([d["wx_b"]] if group else [])
    WTs = [d["wt"].reshape(K, n)] + ([d["wt_b"].reshape(K, n)] if group else [])
    th = _theta_index(it, z)

    J = [np.zeros((n * K, p.n_vars)) for _ in range(P)]
    Jknown = np.ones((n * K, p.n_vars), dtype=bool)
    cons, Jw = [np.zeros(n * K) for _ in range(P)], [np.zeros(n * K) for _ in range(P)]
    JTx = [HP.zeros((N, n)) for _ in range(P)]           # x entries of J' w, per member
    JTth = [HP.zeros((N, z)) for _ in range(P)]          # theta entries (x columns unused), per member
    Hx = [HP.zeros((p.n_vars, p.n_vars)) for _ in range(P)]    # (x, theta) entries, per member
    Ht = [HP.zeros((p.n_vars, p.n_vars)) for _ in range(P)]    # (theta, theta) entries, per member
    xknown = np.zeros(n, dtype=bool)
    xknown[ecols] = True
    norm2 = np.zeros(K)
    for k in range(K):
        u, t, dt, u1 = Zk[k, it.u_off:it.u_off + m], Zk[k, it.t_off], Zk[k, p.dt_idx], Zk[k + 1, it.u_off:it.u_off + m]
        norm2[k] = np.linalg.norm(dt * it.generator(u, t), 2)
        if intervals is not None and k not in intervals:
            continue
        R = T.interval(it.G, it.mods, it.spline_order, it.substeps, np.stack([X[k] for X in Xs], axis=1), u, t, dt, u1,
                       MU=np.stack([M[k] for M in MUs], axis=1), cols=ecols, extra=np.stack([w[k] for w in WXs], axis=1))
        rows = slice(k * n, (k + 1) * n)
        xcol = k * z + it.x_off
        for q in range(P):
            if sampled:
                J[q][rows, xcol:xcol + n] = np.nan
                Jknown[rows, xcol:xcol + n] = False
                Jknown[rows, xcol + ecols] = True
            J[q][rows, xcol + ecols] = -HP.to_float(R["Phi_cols"])
            J[q][rows, (k + 1) * z + it.x_off:(k + 1) * z + it.x_off + n] = np.eye(n)
            cons[q][rows] = HP.to_float(HP.fx(Xs[q][k + 1]) - R["y"][:, q])
            y = HP.fx(WXs[q][k + 1]) - R["extra"][:, q]
            wtf = HP.fx(WTs[q][k])
            for b, cb in enumerate(th):
                col = R["dth"][b][:, q]
                J[q][rows, k * z + cb] = -HP.to_float(col)
                y = y - HP.scale(int(HP.fx(W.reshape(-1)[k * z + cb])), col)
                kk, cc = divmod(k * z + cb, z)
                JTth[q][kk, cc] = JTth[q][kk, cc] - T._dot(col, wtf)
            Jw[q][rows] = HP.to_float(y)
            JTx[q][k, ecols] = JTx[q][k, ecols] - HP.mul(wtf, R["Phi_cols"])
            JTx[q][k + 1] = JTx[q][k + 1] + wtf
            for i, c in enumerate(ecols):
                for b, cb in enumerate(th):
                    Hx[q][xcol + c, k * z + cb] = Hx[q][k * z + cb, xcol + c] = -int(R["Hxth"][q, i, b])
            for a, ca in enumerate(th):
                for b, cb in enumerate(th):
                    Ht[q][k * z + ca, k * z + cb] = Ht[q][k * z + ca, k * z + cb] - int(R["Hthth"][q, a, b])
    Hknown = np.ones((p.n_vars, p.n_vars), dtype=bool)
    JTknown = np.ones((N, z), dtype=bool)
    if sampled:
        JTknown[:K, xs] = xknown[None, :]
        for k in range(K):
            unknown = k * z + it.x_off + np.flatnonzero(~xknown)
            for cb in th:
                Hknown[unknown, k * z + cb] = Hknown[k * z + cb, unknown] = False

    def jtw(q, summed):
        v = JTth[q] + 0
        if summed:
            v = v + JTth[1 - q]
        v[:, xs] = JTx[q]
        out = HP.to_float(v)
        out[~JTknown] = np.nan
        return out.reshape(-1)

    def hess(q, summed):
        M = Hx[q] + Ht[q]
        if summed:
            M = M + Ht[1 - q]
        out = HP.to_float(M[ev_o.hess_rows, ev_o.hess_cols])
        out[~Hknown[ev_o.hess_rows, ev_o.hess_cols]] = np.nan
        return out

    jac = lambda q: J[q][ev_o.jac_rows, ev_o.jac_cols]
    out = dict(cons=cons[0], jac=jac(0), Jw=Jw[0], JTw=jtw(0, False), hess=hess(0, False), norm2=norm2)
    if sampled:
        out.update(cols=cols, jac_known=Jknown[ev_o.jac_rows, ev_o.jac_cols], JTw_known=JTknown.reshape(-1),
                   hess_known=Hknown[ev_o.hess_rows, ev_o.hess_cols])
        assert np.array_equal(np.isfinite(out["jac"]), out["jac_known"])
    if group:
        out.update(JTw_g=jtw(0, True), hess_g=hess(0, True), cons_b=cons[1], jac_b=jac(1), Jw_b=Jw[1], JTw_b=jtw(1, True),
                   hess_b=hess(1, True))
    return out


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        return {k: f[k] for k in f.files}


# ---- the two-member group of a `group` case -------------------------------------------------------------------------------------


def member_fix(fix, q):
    """The fixture as member q of the group sees it (q = 0: x and mu of the fixture, q = 1: x_b, mu_b), in the one-member layout,
    with the entries both members add to summed."""
    out = dict(fix)
    if q == 0:
        out.update(JTw=fix["JTw_g"], hess=fix["hess_g"])
        return out
    n = fix["x_b"].shape[1]
    z = fix["Z"].size // N_KNOTS
    Zk, W = fix["Z"].reshape(N_KNOTS, z).copy(), fix["w"].reshape(N_KNOTS, z).copy()
    Zk[:, :n], W[:, :n] = fix["x_b"], fix["wx_b"]
    out.update(Z=Zk.reshape(-1), w=W.reshape(-1), mu=fix["mu_b"], wt=fix["wt_b"], cons=fix["cons_b"], jac=fix["jac_b"], Jw=fix["Jw_b"],
               JTw=fix["JTw_b"], hess=fix["hess_b"])
    return out


def group_problem(name, fix):
    """(oracle problem of two members x_a, x_b on the components x_a[n], x_b[n], u[m], t, dt; its Z, mu, w, wt)."""
    p1 = problem(name)
    it = p1.integrators[0]
    n, m, z, N = it.x_dim, it.u_dim, p1.z, p1.N
    zg = z + n
    Zk, W = fix["Z"].reshape(N, z), fix["w"].reshape(N, z)
    Zg = np.concatenate([Zk[:, :n], fix["x_b"], Zk[:, n:]], axis=1)
    Wg = np.concatenate([W[:, :n], fix["wx_b"], W[:, n:]], axis=1)
    integ = [O.TimeDependentBilinearIntegrator(q * n, n, 2 * n, m, zg - 2, it.G, it.mods, it.spline_order, it.substeps).bind(zg, zg - 1)
             for q in range(2)]
    pg = O.Problem(N=N, z=zg, dt_idx=zg - 1, integrators=integ, objectives=[O.QuadraticRegularizer(2 * n, m, np.ones(m))],
                   Z0=Zg.reshape(-1).copy())
    return pg, dict(Z=pg.Z0.copy(), mu=np.concatenate([fix["mu"], fix["mu_b"]]), w=Wg.reshape(-1).copy(),
                    wt=np.concatenate([fix["wt"], fix["wt_b"]]))


def member_got(name, fix, got, q):
    """Member q's part of the two-member problem's vectors `got` (any of cons, jac, Jw, JTw, hess; in the structure of
    group_problem's OracleEvaluator), in the one-member structure."""
    p1, ev1 = at_point(name, fix["Z"])
    pg, _ = group_problem(name, fix)
    evg = O.OracleEvaluator(pg)
    n, z, N, K = p1.integrators[0].x_dim, p1.z, p1.N, p1.K
    zg = pg.z
    cmap = np.array([k * zg + (q * n + c if c < n else c + n) for k in range(N) for c in range(z)])
    rows = slice(q * n * K, (q + 1) * n * K)
    out = {}
    for key in ("cons", "Jw"):
        if key in got:
            out[key] = np.asarray(got[key])[rows]
    if "JTw" in got:
        out["JTw"] = np.asarray(got["JTw"])[cmap]
    if "jac" in got:
        Jd = HC._dense(evg.jac_rows, evg.jac_cols, got["jac"], (2 * n * K, pg.n_vars))
        out["jac"] = Jd[rows][:, cmap][ev1.jac_rows, ev1.jac_cols]
    if "hess" in got:
        Hd = HC._dense(evg.hess_rows, evg.hess_cols, got["hess"], (pg.n_vars, pg.n_vars))
        Hd = np.triu(Hd) + np.triu(Hd, 1).T
        out["hess"] = Hd[np.ix_(cmap, cmap)][ev1.hess_rows, ev1.hess_cols]
    return out


# ---- the metric -------------------------------------------------------------------------------------------------------------------


def nerr(a, b, known=None):
    """max|a - b| / max|b| over the known entries; inf if any entry of `a`, known or not, is not finite (a missing writer must not
    pass).  A class whose reference is zero throughout (the t_k column of a family without carriers) is 0 or inf."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        return np.inf
    if known is not None:
        a, b = a[known], b[known]
    d = np.abs(a - b)
    top = np.abs(b).max()
    if top == 0.0:
        return 0.0 if d.max() == 0.0 else np.inf
    return float(d.max() / top)


def errors(name, fix, got):
    """{(class, k): normwise error} of the vectors in `got` (any of cons, jac, Jw, JTw, hess) against the fixture `fix`.  Per
    interval k: "defect" (scaled by max|Phi x_k|), "Phi", "u0".. (u_k columns), "t", "dt", "un0".. (u_{k+1} columns, order 1),
    "const" (the identity and the zeros of the two-knot block, exactly), "Jw" (the interval's rows), "hess" (the two-knot window
    of the interval; neighbouring windows share the knot between them); per knot k = 0 .. N-1: "JTw"."""
    p, ev_o = at_point(name, fix["Z"])
    it = p.integrators[0]
    n, m, z, K = it.x_dim, it.u_dim, p.z, p.K
    Zk = fix["Z"].reshape(p.N, z)
    order1 = it.spline_order == 1
    out = {}
    if "cons" in got:
        for k in range(K):
            rows = slice(k * n, (k + 1) * n)
            y = Zk[k + 1, it.x_off:it.x_off + n] - fix["cons"][rows]
            d = np.abs(np.asarray(got["cons"])[rows] - fix["cons"][rows])
            out[("defect", k)] = float(d.max() / np.abs(y).max()) if np.all(np.isfinite(d)) else np.inf
    if "jac" in got:
        shape = (n * K, p.n_vars)
        Ja, Jb = HC._dense(ev_o.jac_rows, ev_o.jac_cols, got["jac"], shape), HC._dense(ev_o.jac_rows, ev_o.jac_cols, fix["jac"], shape)
        Kn = HC._dense(ev_o.jac_rows, ev_o.jac_cols, fix["jac_known"], shape).astype(bool) if "jac_known" in fix else np.ones(shape, dtype=bool)
        for k in range(K):
            rows = slice(k * n, (k + 1) * n)
            xs = slice(k * z + it.x_off, k * z + it.x_off + n)
            out[("Phi", k)] = nerr(Ja[rows, xs], Jb[rows, xs], Kn[rows, xs])
            named = [(f"u{j}", k * z + it.u_off + j) for j in range(m)] + [("t", k * z + it.t_off), ("dt", k * z + p.dt_idx)]
            if order1:
                named += [(f"un{j}", (k + 1) * z + it.u_off + j) for j in range(m)]
            for cls, col in named:
                out[(cls, k)] = nerr(Ja[rows, col], Jb[rows, col])
            rest_a, rest_b = Ja[rows, k * z:(k + 2) * z].copy(), Jb[rows, k * z:(k + 2) * z].copy()
            for M in (rest_a, rest_b):
                M[:, it.x_off:it.x_off + n] = 0.0
                for _, col in named:
                    M[:, col - k * z] = 0.0
            out[("const", k)] = 0.0 if np.array_equal(rest_a, rest_b) else np.inf
    if "Jw" in got:
        for k in range(K):
            rows = slice(k * n, (k + 1) * n)
            out[("Jw", k)] = nerr(np.asarray(got["Jw"])[rows], fix["Jw"][rows])
    if "JTw" in got:
        kn = fix["JTw_known"] if "JTw_known" in fix else np.ones(p.n_vars, dtype=bool)
        for k in range(p.N):
            s = slice(k * z, (k + 1) * z)
            out[("JTw", k)] = nerr(np.asarray(got["JTw"])[s], fix["JTw"][s], kn[s])
    if "hess" in got:
        shape = (p.n_vars, p.n_vars)
        Ha, Hb = HC._dense(ev_o.hess_rows, ev_o.hess_cols, got["hess"], shape), HC._dense(ev_o.hess_rows, ev_o.hess_cols, fix["hess"], shape)
        Kn = HC._dense(ev_o.hess_rows, ev_o.hess_cols, fix["hess_known"], shape).astype(bool) if "hess_known" in fix else np.ones(shape, dtype=bool)
        inside = np.zeros(shape, dtype=bool)
        for k in range(K):
            s = slice(k * z, (k + 2) * z)
            inside[s, s] = True
            out[("hess", k)] = nerr(Ha[s, s], Hb[s, s], Kn[s, s])
        out[("hess_outside_blocks", 0)] = 0.0 if not np.any(Ha[~inside] != 0.0) else np.inf   # (NaN != 0 is True)
    return out


def report(name, fix, errs, extra=""):
    """The errors as text, one line per interval: ||dt_k G(u_k, t_k)||_2 beside every class."""
    K = len(fix["norm2"])
    classes = sorted({c for c, _ in errs})
    lines = [f"{name} {extra}"]
    for k in range(K + 1):
        cells = [f"{c}={errs[(c, k)]:.2e}" for c in classes if (c, k) in errs]
        if cells:
            head = f"  k={k} |dt G|2={fix['norm2'][k]:5.2f}" if k < K else f"  k={k} (last knot)"
            lines.append(head + "  " + " ".join(cells))
    return "\n".join(lines)


# ---- the yardstick and the bars ---------------------------------------------------------------------------------------------------

EXACT = ("const", "hess_outside_blocks")


def callbacks_of(ev, d):
    """The five vectors of an oracle-style evaluator at the inputs d."""
    Z = d["Z"]
    return dict(cons=ev.eval_constraint(Z), jac=ev.eval_constraint_jacobian(Z), Jw=ev.eval_constraint_jacobian_product(Z, d["w"]),
                JTw=ev.eval_constraint_jacobian_transpose_product(Z, d["wt"]), hess=ev.eval_hessian_lagrangian(Z, 0.0, d["mu"]))


def yardstick_errors(name, fix, integrator_class=None):
    """{(class, k): error} of tests/tdb_large_cases.py's fp64 restatement against the fixture: the one-member problem, and for a
    `group` case both members of the two-member problem as well (the worst of the three per class and interval).
    `integrator_class`: a subclass of L.FastTdb to put in its place (the perturbation tests)."""
    import dataclasses

    def fast(p):
        q = L.fast_problem(p)
        if integrator_class is not None:
            q = dataclasses.replace(q, integrators=[integrator_class(**{f.name: getattr(i, f.name) for f in dataclasses.fields(i)})
                                                    for i in q.integrators])
        return q

    p, _ = at_point(name, fix["Z"])
    errs = errors(name, fix, callbacks_of(O.OracleEvaluator(fast(p)), fix))
    if CASES[name].get("group") and integrator_class is None:
        pg, dg = group_problem(name, fix)
        got = callbacks_of(O.OracleEvaluator(fast(pg)), dg)
        for q in range(2):
            for key, v in errors(name, member_fix(fix, q), member_got(name, fix, got, q)).items():
                errs[key] = max(errs[key], v)
    return errs


def bars_from(errs):
    """(classes, yard (classes x N_KNOTS, NaN where a class has no entry), bars) of yardstick errors."""
    classes = sorted({c for c, _ in errs})
    yard = np.full((len(classes), N_KNOTS), np.nan)
    for (c, k), v in errs.items():
        yard[classes.index(c), k] = v
    bars = np.array([0.0 if c in EXACT else max(BAR_FACTOR * np.nanmax(yard[i]), HC.BAR_NO_SQUARING) for i, c in enumerate(classes)])
    return np.array(classes), yard, bars


def bar_for(fix, cls):
    """The bar of a class, as the fixture stores it."""
    i = list(fix["classes"]).index(cls)
    return float(fix["bars"][i])
