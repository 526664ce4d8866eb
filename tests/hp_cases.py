"""The cases of the accuracy-budget tests (tests/test_hp_reference.py, tests/test_gpu_accuracy_budget.py): problems rebuilt from
their seeds, the dt ladder, the expected callback vectors from tests/hp_reference.py laid out in the oracle's structure, and the
metric -- the NORMWISE error per interval and quantity class, max|a - b| / max|b| over the entries of the class in that interval.

One BilinearIntegrator per problem (the DerivativeIntegrator of the scaling generator is dropped: it has no exponential), seven
knots, skew-symmetric generators, and dt_k chosen so that ||A_k||_2 walks the ladder below in shuffled knot order.

From 130 states on (`sample_E` in CASES) a whole E_k = exp(A_k) is out of the reference's reach (minutes per interval, 500 KB per
fixture), so the expected Jacobian holds 16 sampled columns of each E_k block -- the same columns in every interval, as the action
of exp(A_k) on unit vectors -- and NaN elsewhere in the block; the fixture's `jac_known` marks what is known, and the "E" class is
measured over those entries alone (every other entry of the block must still be a number).  Every u_j column, dt column, identity and structural zero is known and checked as before.  The
rest of the block is still exercised in aggregate: J w and J' w contract all of it with random vectors, and on the value-slab route
(tests/test_gpu_accuracy_budget.py) they contract the engine's own stored E_k entries."""
import hashlib
import os

import numpy as np

import dto_oracle as O
import hp_reference as HP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LADDER = (0.5, 4.0, 8.0, 11.0, 14.0, 20.0)   # ||A_k||_2: no squaring / the chain's radii / one round / q = 1 -> 2 / several rounds
N_KNOTS = 7
Q1_TOP = 6.0        # hp_ring256_q1: the largest of 6, 5, 4, 3 at which every callback's sweeps run one round
CASES = {
    "hp_small": dict(kind="dense", n=9, m=2, seed=901),       # k_small
    "hp_s64": dict(kind="dense", n=40, m=2, seed=902),        # k_chain64 + k_sweep_s64
    # npad = 128: batched chain, planner's sweep.  Top rung 24, not 20: the planner bounds the growth rate in the 1-norm, which
    # is pessimistic for skew matrices, so with 20 a theta_v of 14 still left two rounds of radius 10 and stayed under the bar;
    # at 24 it runs two rounds of radius 12 (over the bar) where theta_v = 9 runs three of radius 8
    "hp_general": dict(kind="dense", n=66, m=1, seed=903, ladder=(0.5, 4.0, 8.0, 11.0, 14.0, 24.0)),
    "hp_kron": dict(kind="kron", b=16, r=4, m=2, seed=904),   # dto_kron.hip (block_generators=True)
    # npad = 192: three 64-tiles a side in the chain's GEMM, no one-launch sweep form (step launches only)
    "hp_tile192": dict(kind="dense", n=130, m=1, seed=905, ladder=(0.5, 4.0, 8.0, 11.0, 14.0, 24.0), sample_E=16),
    # npad = 256, the benchmark's size: the ring GEMM on 2 x 2 tiles with 6 dead rows; sub-stepped sweeps, non-pairing Hessian
    "hp_ring256": dict(kind="dense", n=250, m=2, seed=906, ladder=(0.5, 4.0, 8.0, 11.0, 14.0, 24.0), sample_E=16),
    # ... and the same chain with every sweep in one round: the generator-stationary form, the pairing Hessian (DESIGN section 2
    # records how the top rung was chosen)
    "hp_ring256_q1": dict(kind="dense", n=250, m=2, seed=907, ladder=(0.5, 1.0, 2.0, 3.0, 4.0, Q1_TOP), sample_E=16),
    # npad = 384: the ring GEMM's odd 3 x 3 tile walk with 54 dead rows, step-launch sweeps beside the chain
    "hp_ring384": dict(kind="dense", n=330, m=1, seed=908, ladder=(0.5, 4.0, 8.0, 11.0, 14.0, 24.0), sample_E=16),
}
ENGINE_KW = {"hp_kron": dict(block_generators=True)}

BAR = 2.0 * np.exp(9.0) * 2.0 ** -53        # values, Jacobian classes, J w, J' w: theta_v = 9 e-folds on a Taylor sum, doubled
BAR_H = 4.0 * np.exp(9.0) * 2.0 ** -53      # Hessian block: a forward and an adjoint budget add
BAR_NO_SQUARING = 64.0 * 2.0 ** -53         # E_k inside the radius (||A||_2 = 0.5)
ORACLE_CAP = 1e-13


def problem(name):
    """The case's oracle problem at its seed's point (dt = 0.1 everywhere; `ladder` sets the steps)."""
    c = CASES[name]
    if c["kind"] == "dense":
        p = O.make_scaled_problem(N_KNOTS, c["n"], c["m"], seed=c["seed"], skew=True)
        p.integrators = p.integrators[:1]
        return p
    b, r, m = c["b"], c["r"], c["m"]
    rng = np.random.default_rng(c["seed"])
    n = b * r
    B = rng.standard_normal((m + 1, b, b))
    B = (B - B.transpose(0, 2, 1)) / np.sqrt(2.0 * b)
    G = np.stack([np.kron(np.eye(r), Bj) for Bj in B])
    z = n + 2 * m + 1
    Zk = rng.standard_normal((N_KNOTS, z))
    Zk[:, n:n + m] *= 0.3
    Zk[:, z - 1] = 0.1
    return O.Problem(N=N_KNOTS, z=z, dt_idx=z - 1, integrators=[O.BilinearIntegrator(0, n, n, m, G)],
                     objectives=[O.QuadraticRegularizer(n, m, np.ones(m))], Z0=Zk.reshape(-1).copy())


def _block(name, p):
    """(generators the reference exponentiates, segments they act on alike)."""
    it = p.integrators[0]
    if CASES[name]["kind"] == "kron":
        b, r = CASES[name]["b"], CASES[name]["r"]
        return it.G[:, :b, :b].copy(), r
    return it.G, 1


def ladder(name, p):
    """(Z, dt): the seed's point with dt_k = rung[perm[k]] / ||G(u_k)||_2 (the case's own ladder, else LADDER); the last knot's own step stays 0.1."""
    it = p.integrators[0]
    G, _ = _block(name, p)
    Zk = p.Z0.reshape(p.N, p.z).copy()
    rungs = CASES[name].get("ladder", LADDER)
    perm = np.random.default_rng(CASES[name]["seed"] + 7).permutation(len(rungs))
    for k in range(p.K):
        u = Zk[k, it.u_off:it.u_off + it.u_dim]
        Gu = G[0] + np.tensordot(u, G[1:], axes=(0, 0))
        Zk[k, p.dt_idx] = rungs[perm[k]] / np.linalg.norm(Gu, 2)
    return Zk.reshape(-1).copy(), Zk[:, p.dt_idx].copy()


def E_columns(name):
    """The sampled columns of every E_k block of a `sample_E` case (None for a case whose E_k is known whole): columns 0, 15, 16,
    63, 64, n - 1, both sides of every 128-column boundary below n, and the rest drawn from the case's seed."""
    c = CASES[name]
    if "sample_E" not in c:
        return None
    n = c["n"]
    must = {0, 15, 16, 63, 64, n - 1} | {b + s for b in range(128, n, 128) for s in (-1, 0)}
    rest = [int(j) for j in np.random.default_rng(c["seed"] + 29).permutation(n) if int(j) not in must]
    return np.array(sorted(must | set(rest[:c["sample_E"] - len(must)])), dtype=np.int64)


def inputs(name):
    """Everything a fixture stores that a seed does not give back: Z (with the ladder), mu, w, wt, dt."""
    p = problem(name)
    Z, dt = ladder(name, p)
    rng = np.random.default_rng(CASES[name]["seed"] + 13)
    n_cons = p.integrators[0].x_dim * p.K
    return dict(Z=Z, dt=dt, mu=rng.standard_normal(n_cons), w=rng.standard_normal(p.n_vars), wt=rng.standard_normal(n_cons))


def input_hash(d):
    h = hashlib.sha256()
    for k in ("Z", "dt", "mu", "w", "wt"):
        h.update(np.ascontiguousarray(d[k], dtype=np.float64).tobytes())
    return h.hexdigest()


def at_point(name, Z):
    """(problem with Z0 = Z, its OracleEvaluator): the structure every vector is laid out in."""
    p = problem(name)
    p.Z0 = np.asarray(Z, dtype=np.float64).copy()
    return p, O.OracleEvaluator(p)


def expected(name, d):
    """The expected callback vectors of the case at the inputs d, computed by tests/hp_reference.py and rounded to fp64:
    cons, jac, Jw, JTw, hess (sigma = 0), and norm2 / norm1 of A_k."""
    p, ev_o = at_point(name, d["Z"])
    it = p.integrators[0]
    n, m, z, K = it.x_dim, it.u_dim, p.z, p.K
    G, r = _block(name, p)
    b = G.shape[1]
    Zk = d["Z"].reshape(p.N, z)
    W = d["w"].reshape(p.N, z)
    xs = slice(it.x_off, it.x_off + n)
    cols = lambda v: np.asarray(v, dtype=np.float64).reshape(r, b).T          # x of n = r b entries -> (b, r) columns
    flat = lambda M: M.T.reshape(-1)                                           # and back, fixed point or float
    loc = np.concatenate([np.arange(it.x_off, it.x_off + n), np.arange(it.u_off, it.u_off + m), [p.dt_idx]])
    ecols = E_columns(name)       # None: the whole E_k; else the sampled columns, everything else of the block NaN / unknown
    assert ecols is None or r == 1
    J = np.zeros((n * K, p.n_vars))
    known = np.ones(J.shape, dtype=bool)
    Hd = np.zeros((p.n_vars, p.n_vars))
    cons, Jw = np.zeros(n * K), np.zeros(n * K)
    JTw = HP.zeros((p.N, z))
    for k in range(p.N):
        JTw[k] = HP.fx(np.zeros(z))
    norm2, norm1 = np.zeros(K), np.zeros(K)
    for k in range(K):
        u, dt = Zk[k, it.u_off:it.u_off + m], Zk[k, p.dt_idx]
        R = HP.interval(G, cols(Zk[k, xs]), u, dt, cols(Zk[k + 1, xs]), mu=cols(d["mu"][k * n:(k + 1) * n]),
                        want_E=ecols is None, E_cols=ecols)
        A = HP.to_float(R["A"])
        norm2[k], norm1[k] = np.linalg.norm(A, 2), np.linalg.norm(A, 1)
        rows = slice(k * n, (k + 1) * n)
        WT = HP.fx(cols(d["wt"][rows]))
        if ecols is None:
            J[rows, k * z + it.x_off:k * z + it.x_off + n] = -np.kron(np.eye(r), HP.to_float(R["E"]))
            Ew, ETwt = HP.mul(R["E"], HP.fx(cols(W[k, xs]))), HP.mul(R["E"].T.copy(), WT)
        else:
            J[rows, k * z + it.x_off:k * z + it.x_off + n] = np.nan
            known[rows, k * z + it.x_off:k * z + it.x_off + n] = False
            J[rows, k * z + it.x_off + ecols] = -HP.to_float(R["E_cols"])
            known[rows, k * z + it.x_off + ecols] = True
            Ew, ETwt = HP.expm_action(R["A"], HP.fx(cols(W[k, xs]))), HP.expm_action(R["A"].T.copy(), WT)
        for j in range(m):
            J[rows, k * z + it.u_off + j] = -flat(HP.to_float(R["LX"][j]))
        J[rows, k * z + p.dt_idx] = -flat(HP.to_float(R["GEX"]))
        J[rows, (k + 1) * z + it.x_off:(k + 1) * z + it.x_off + n] = np.eye(n)
        cons[rows] = flat(HP.to_float(R["defect"]))
        # J w of the interval's rows and the interval's part of J' w, in fixed point, rounded once
        y = HP.fx(cols(W[k + 1, xs])) - Ew - HP.scale(int(HP.fx(W[k, p.dt_idx])), R["GEX"])
        for j in range(m):
            y = y - HP.scale(int(HP.fx(W[k, it.u_off + j])), R["LX"][j])
        Jw[rows] = flat(HP.to_float(y))
        JTw[k, xs] = JTw[k, xs] - flat(ETwt)
        JTw[k + 1, xs] = JTw[k + 1, xs] + flat(WT)
        for j in range(m):
            JTw[k, it.u_off + j] = -HP._dot(R["LX"][j], WT)
        JTw[k, p.dt_idx] = -HP._dot(R["GEX"], WT)
        Hd[np.ix_(k * z + loc, k * z + loc)] += HP.to_float(R["H"])
    out = dict(cons=cons, jac=J[ev_o.jac_rows, ev_o.jac_cols], Jw=Jw, JTw=HP.to_float(JTw).reshape(-1),
               hess=Hd[ev_o.hess_rows, ev_o.hess_cols], norm2=norm2, norm1=norm1)
    assert np.count_nonzero(J) == np.count_nonzero(out["jac"]) and np.count_nonzero(np.triu(Hd)) == np.count_nonzero(out["hess"])
    if ecols is not None:
        out["jac_known"] = known[ev_o.jac_rows, ev_o.jac_cols]
        out["E_cols"] = ecols
        assert np.array_equal(np.isfinite(out["jac"]), out["jac_known"])
    return out


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        return {k: f[k] for k in f.files}


# ---- the metric ---------------------------------------------------------------------------------------------------------------


def nerr(a, b):
    """max|a - b| / max|b| (NaN in `a` gives inf: a missing writer must not pass)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.abs(a - b)
    if not np.all(np.isfinite(d)):
        return np.inf
    return float(d.max() / np.abs(b).max())


def _dense(rows, cols, vals, shape):
    M = np.zeros(shape)
    M[rows, cols] = vals
    return M


def errors(name, fix, got):
    """{(class, k): normwise error} of the vectors in `got` (any of cons, jac, Jw, JTw, hess) against the fixture `fix`.
    Jacobian classes per interval k: "E", "u0".., "dt"; "defect" is scaled by max|E_k x_k|; "Jw" the interval's rows, "JTw" the
    knot's columns (k = 0 .. N-1), "hess" the interval's block."""
    p, ev_o = at_point(name, fix["Z"])
    it = p.integrators[0]
    n, m, z, K = it.x_dim, it.u_dim, p.z, p.K
    Zk = fix["Z"].reshape(p.N, z)
    out = {}
    if "cons" in got:
        for k in range(K):
            rows = slice(k * n, (k + 1) * n)
            Ex = Zk[k + 1, it.x_off:it.x_off + n] - fix["cons"][rows]
            d = np.abs(np.asarray(got["cons"])[rows] - fix["cons"][rows])
            out[("defect", k)] = float(d.max() / np.abs(Ex).max()) if np.all(np.isfinite(d)) else np.inf
    if "jac" in got:
        shape = (n * K, p.n_vars)
        Ja, Jb = _dense(ev_o.jac_rows, ev_o.jac_cols, got["jac"], shape), _dense(ev_o.jac_rows, ev_o.jac_cols, fix["jac"], shape)
        # sampled E_k (jac_known): the "E" class over the known entries only -- unknown ones sit nowhere but in the E_k blocks
        Kn = _dense(ev_o.jac_rows, ev_o.jac_cols, fix["jac_known"], shape).astype(bool) if "jac_known" in fix else None
        for k in range(K):
            rows = slice(k * n, (k + 1) * n)
            xs = slice(k * z + it.x_off, k * z + it.x_off + n)
            if Kn is None:
                out[("E", k)] = nerr(Ja[rows, xs], Jb[rows, xs])
            else:   # (a missing writer must not pass in the unsampled columns either: every entry of the block is a number)
                out[("E", k)] = nerr(Ja[rows, xs][Kn[rows, xs]], Jb[rows, xs][Kn[rows, xs]]) if np.all(np.isfinite(Ja[rows, xs])) else np.inf
            for j in range(m):
                out[(f"u{j}", k)] = nerr(Ja[rows, k * z + it.u_off + j], Jb[rows, k * z + it.u_off + j])
            out[("dt", k)] = nerr(Ja[rows, k * z + p.dt_idx], Jb[rows, k * z + p.dt_idx])
            # what is left of the two-knot block: zeros and the identity of the x_{k+1} half, exactly
            rest_a, rest_b = Ja[rows, k * z:(k + 2) * z].copy(), Jb[rows, k * z:(k + 2) * z].copy()
            for M in (rest_a, rest_b):
                M[:, it.x_off:it.x_off + n] = 0.0
                M[:, it.u_off:it.u_off + m] = 0.0
                M[:, p.dt_idx] = 0.0
            out[("const", k)] = 0.0 if np.array_equal(rest_a, rest_b) else np.inf
    if "Jw" in got:
        for k in range(K):
            rows = slice(k * n, (k + 1) * n)
            out[("Jw", k)] = nerr(np.asarray(got["Jw"])[rows], fix["Jw"][rows])
    if "JTw" in got:
        for k in range(p.N):
            out[("JTw", k)] = nerr(np.asarray(got["JTw"])[k * z:(k + 1) * z], fix["JTw"][k * z:(k + 1) * z])
    if "hess" in got:
        shape = (p.n_vars, p.n_vars)
        Ha, Hb = _dense(ev_o.hess_rows, ev_o.hess_cols, got["hess"], shape), _dense(ev_o.hess_rows, ev_o.hess_cols, fix["hess"], shape)
        for k in range(K):
            s = slice(k * z, (k + 1) * z)
            out[("hess", k)] = nerr(Ha[s, s], Hb[s, s])
        off = Ha - Hb
        for k in range(K):
            off[k * z:(k + 1) * z, k * z:(k + 1) * z] = 0.0
        out[("hess_outside_blocks", 0)] = 0.0 if not np.any(off != 0.0) else np.inf   # (NaN != 0 is True)
    return out


def report(name, fix, errs, extra=""):
    """The errors as text, one line per interval: ||A_k||_2 beside every class."""
    K = len(fix["norm2"])
    classes = sorted({c for c, _ in errs})
    lines = [f"{name} {extra}"]
    for k in range(K + 1):
        cells = [f"{c}={errs[(c, k)]:.2e}" for c in classes if (c, k) in errs]
        if cells:
            head = f"  k={k} |A|2={fix['norm2'][k]:5.2f} |A|1={fix['norm1'][k]:6.2f}" if k < K else f"  k={k} (last knot)"
            lines.append(head + "  " + " ".join(cells))
    return "\n".join(lines)


def bar_for(cls):
    if cls in ("const", "hess_outside_blocks"):
        return 0.0
    return BAR_H if cls == "hess" else BAR
