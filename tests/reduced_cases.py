"""Shared by the tests of the reduced-space operators (dto_reduced_gradient, dto_reduced_hessian_product; csrc/dto_reduced.hip,
csrc/dto_reduced_plan.h): the dense reference built from the ORACLE alone, the composition of the operators out of the Evaluator's
existing public methods with NumPy indexing, and the cases.

Sets: S, the dependent entries of Z (the state components of every integrator at knots 2 .. N); C, every other entry.  With
J_S / J_C the dynamics rows of the oracle's Jacobian in the columns S / C and g = sigma grad f + J_con' mu_con:
    T      identity rows on C, -J_S^-1 J_C on S            (the tangent map of the feasible manifold)
    lam    -J_S^-T g_S                                     (multipliers of the dynamics rows: mu~_dyn)
    r_ref  T' g          y_ref  T' H(Z; sigma, [lam; mu_con]) T v
The reference's `mistake` argument breaks it in one named way, for the test that shows the bar can fail.

Accuracy bar: the Hessian is held to 1e-8 against the oracle (helpers.TOL_H) and y is its linear image, so
    ||y - y_ref||_2 <= 1e-8 ||T||_2^2 ||H||_2 ||v||_2;        gradient:  ||r - r_ref||_2 <= 1e-10 levels ||T||_2^2 ||g||_2
(1e-10 levels: the whole-dynamics solves' bar), every factor from the dense reference.  Condition on the cases:
kappa = ||T||_2^2 ||H||_2 ||v||_2 / ||y_ref||_2 <= 1e4, so the bar never exceeds 1e-4 relative."""
import functools

import numpy as np
import scipy.sparse as sp

import dto_oracle as O
from elim_cases import dense_jacobian, describe, plan, three_level_problem
from helpers import TOL, TOL_H, to_engine
from multi_ket_cases import multi_ket, to_oracle
from test_gpu_block_generators import kron_problem

KAPPA_CAP = 1e4
SIGMA = 0.7

CASES = ["scaled_12x9", "scaled_40x6", "scaled_70x5", "three_level_12x6", "three_level_40x6", "multi_ket_between", "tdb_order0", "tdb_order1",
         "structured_16x4", "scaled_12x9+con", "scaled_40x6+con"]
SMALL_CASES = ["scaled_12x9", "scaled_12x9+con", "three_level_12x6", "multi_ket_between_6", "tdb_order0", "tdb_order1"]   # what the CPU tests afford


def problem(name):
    """a fresh oracle problem with the terminal objective on the first integrator's states, and the Evaluator keywords"""
    con = name.endswith("+con")
    base, kw = (name[:-4] if con else name), {}
    if base.startswith("scaled_"):
        n, N = (int(v) for v in base[7:].split("x"))
        p = O.make_scaled_problem(N, n, 2, seed=300 + n + N, skew=True, with_constraint=con)
    elif base.startswith("three_level_"):
        n, N = (int(v) for v in base[12:].split("x"))
        p = three_level_problem(n, N)
    elif base.startswith("multi_ket_between"):
        p, kw = to_oracle(multi_ket(6 if base.endswith("_6") else 40, 2, 5, derivative_between=True)), dict(shared_generators=True)
    elif base in ("tdb_order0", "tdb_order1"):
        p = O.make_tdb_problem(N=6, n=4, m=2, order=int(base[-1]), substeps=16, with_derivative=True)
    elif base == "structured_16x4":
        p, kw = kron_problem(16, 4, 2, 5, seed=3), dict(block_generators=True)
    else:
        raise KeyError(name)
    it = p.integrators[0]
    goal = np.random.default_rng(3).standard_normal((1, it.x_dim))
    if p.weights is not None:
        p.weights = list(p.weights) + [1.0]
    p.objectives = list(p.objectives) + [O.KnotSqDistObjective(list(range(it.x_off, it.x_off + it.x_dim)), [p.N], [1.0], goal)]
    return p, kw


# ------------------------------------------------------------------------------------------------------------ index sets
def index_sets(p):
    """S (dependent entries), C (the others), S0 (the states of knot 1), all ascending; per integrator its D-axis offset"""
    its = describe(p)
    state = np.zeros(p.n_vars, dtype=bool)
    sk = state[:p.N * p.z].reshape(p.N, p.z)
    for i in its:
        sk[:, i["x_off"]:i["x_off"] + i["x_dim"]] = True
    dep = state.copy()
    dep[:p.z] = False
    first = state & ~dep
    pre = [sum(i["x_dim"] for i in its[:a]) for a in range(len(its))]
    return np.flatnonzero(dep), np.flatnonzero(~dep), np.flatnonzero(first), pre


def dense_hessian(ev_o, Z, sigma, mu):
    r1, c1 = ev_o.hessian_structure1()
    n = ev_o.prob.n_vars
    U = sp.coo_matrix((ev_o.eval_hessian_lagrangian(Z, sigma, mu), (r1 - 1, c1 - 1)), shape=(n, n)).toarray()   # duplicates summed
    return U + U.T - np.diag(np.diag(U))


def constraint_rows(p, Z):
    """the oracle's Jacobian of the non-dynamics rows, dense: (n_cons - n_dyn, n_vars)"""
    if not p.constraints:
        return np.zeros((0, p.n_vars))
    return np.vstack([O.constraint_jacobian(c, p, Z).toarray() for c in p.constraints])


def reduced_pieces(p, Z, sigma, mu):
    """g, T (n_vars x |C|), lam (dynamics multipliers), everything the reference needs short of the Hessian"""
    S, C, _, _ = index_sets(p)
    Jd = dense_jacobian(p, Z)
    n_dyn = Jd.shape[0]
    Jc = constraint_rows(p, Z)
    mu_c = np.zeros(Jc.shape[0]) if mu is None else np.asarray(mu)[n_dyn:]
    g = sigma * O.objective_gradient(p, Z) + Jc.T @ mu_c
    T = np.zeros((p.n_vars, C.size))
    T[C, np.arange(C.size)] = 1.0
    T[S] = -np.linalg.solve(Jd[:, S], Jd[:, C])
    lam = -np.linalg.solve(Jd[:, S].T, g[S])
    return dict(S=S, C=C, g=g, T=T, lam=lam, mu_c=mu_c, n_dyn=n_dyn)


def reduced_gradient_ref(p, Z, sigma, mu):
    """r_ref as an n_vars vector (zero on S)"""
    q = reduced_pieces(p, Z, sigma, mu)
    r = np.zeros(p.n_vars)
    r[q["C"]] = q["T"].T @ q["g"]
    return r


def shift_one_knot(p, lam):
    """the multipliers of interval k + 1 in the rows of interval k (the last interval keeps its own): the named mistake"""
    out, K, row = lam.copy(), p.N - 1, 0
    for it in p.integrators:
        blk = lam[row:row + K * it.x_dim].reshape(K, it.x_dim)
        out[row:row + K * it.x_dim] = np.vstack([blk[1:], blk[-1:]]).reshape(-1)
        row += K * it.x_dim
    return out


def dense_reference(p, Z, sigma, mu, mistake=None):
    """dict with r_ref, the reduced Hessian Hr on C (|C| x |C|), T, H, g and the norms the bars are made of.
    mistake: None, "zero" (mu~_dyn = 0), "plus" (mu~_dyn = +Lam, i.e. -lam), "shift" (Lam shifted by one knot)"""
    q = reduced_pieces(p, Z, sigma, mu)
    lam = {None: q["lam"], "zero": 0.0 * q["lam"], "plus": -q["lam"], "shift": shift_one_knot(p, q["lam"])}[mistake]
    H = dense_hessian(O.OracleEvaluator(p), Z, sigma, np.concatenate([lam, q["mu_c"]]))
    T = q["T"]
    r = np.zeros(p.n_vars)
    r[q["C"]] = T.T @ q["g"]
    return dict(q, r_ref=r, H=H, Hr=T.T @ H @ T, nT=float(np.linalg.norm(T, 2)), nH=float(np.linalg.norm(H, 2)),
                ng=float(np.linalg.norm(q["g"])), mut=np.concatenate([lam, q["mu_c"]]))


def product_ref(ref, v):
    y = np.zeros(v.size)
    y[ref["C"]] = ref["Hr"] @ v[ref["C"]]
    return y


def product_bar(ref, v):
    return TOL_H * ref["nT"] ** 2 * ref["nH"] * float(np.linalg.norm(v[ref["C"]]))


def gradient_bar(ref, levels):
    return TOL * levels * ref["nT"] ** 2 * ref["ng"]


def kappa(ref, v):
    return ref["nT"] ** 2 * ref["nH"] * float(np.linalg.norm(v[ref["C"]])) / float(np.linalg.norm(product_ref(ref, v)))


def oracle_feasible(p, Z):
    """Z with the dependent entries moved onto the feasible manifold: Newton on the dynamics rows in the columns S (the block is
    triangular in dependency order, so a handful of steps end at rounding level); the oracle alone"""
    S = index_sets(p)[0]
    Z = np.array(Z, dtype=np.float64)
    for _ in range(12):
        c = np.concatenate([O.integrator_evaluate(it, p, Z) for it in p.integrators])
        if np.max(np.abs(c)) <= 1e-13:
            break
        Z[S] -= np.linalg.solve(dense_jacobian(p, Z)[:, S], c)
    return Z


def free_direction(p, rng):
    d = rng.standard_normal(p.n_vars)
    d[index_sets(p)[0]] = 0.0
    return d


@functools.lru_cache(maxsize=None)
def case(name):
    """oracle problem, engine problem, Evaluator keywords, the point, mu (None, or random on the constraint rows), the dense reference at
    sigma = SIGMA and two directions with their reference products: computed once, shared, never written"""
    p, kw = problem(name)
    Z = np.ascontiguousarray(p.Z0, dtype=np.float64)
    n_dyn = sum(it.x_dim for it in p.integrators) * (p.N - 1)
    n_cons = n_dyn + sum(c.g_dim * len(c.times1) for c in p.constraints)
    mu = None
    if name.endswith("+con"):
        mu = np.zeros(n_cons)
        mu[n_dyn:] = np.random.default_rng(11).standard_normal(n_cons - n_dyn)
    ref = dense_reference(p, Z, SIGMA, mu)
    rng = np.random.default_rng(len(name))
    vs = [rng.standard_normal(p.n_vars) for _ in range(2)]
    ys = [product_ref(ref, v) for v in vs]
    for a in [Z] + vs + ys + ([mu] if mu is not None else []) + [x for x in ref.values() if isinstance(x, np.ndarray)]:
        a.setflags(write=False)
    return dict(p=p, pe=to_engine(p), kw=kw, Z=Z, mu=mu, ref=ref, vs=vs, ys=ys, levels=plan(describe(p), p.dt_idx, p.N - 1)["n_levels"],
                n_cons=n_cons, n_dyn=n_dyn)


# ----------------------------------------------------------------------------- the composition: today's public methods and NumPy
def _layout(ev, p):
    D, _, offset, _ = ev.dynamics_layout()
    K = p.N - 1
    return D, [int(o) for o in offset], [K * int(o) for o in offset]   # row0_i = (N - 1) pre_i


def pack_states(p, offset, D, x):
    """the state entries of a Z-layout vector as (N, 1, D)"""
    xk = x[:p.N * p.z].reshape(p.N, p.z)
    B = np.zeros((p.N, 1, D))
    for i, it in enumerate(p.integrators):
        B[:, 0, offset[i]:offset[i] + it.x_dim] = xk[:, it.x_off:it.x_off + it.x_dim]
    return B


def dynamics_rows(p, offset, row0, n_cons, L):
    """w (n_cons): L[1:] (L: (N, D)) in the dynamics rows, zero elsewhere"""
    w = np.zeros(n_cons)
    for i, it in enumerate(p.integrators):
        w[row0[i]:row0[i] + (p.N - 1) * it.x_dim] = L[1:, offset[i]:offset[i] + it.x_dim].reshape(-1)
    return w


def finish(p, offset, q, t, L):
    y = q - t
    yk = y[:p.N * p.z].reshape(p.N, p.z)
    for i, it in enumerate(p.integrators):
        yk[:, it.x_off:it.x_off + it.x_dim] = 0.0
        yk[0, it.x_off:it.x_off + it.x_dim] = L[0, offset[i]:offset[i] + it.x_dim]
    return y


def compose_gradient(ev, p, Z, sigma, mu):
    """(r, Lam (N, D), mu~) by the recipe of dto_reduced_gradient"""
    D, offset, row0 = _layout(ev, p)
    n_dyn = ev.n_dynamics_constraints
    g = np.full(ev.n_variables, np.nan)
    ev.eval_objective_gradient(g, Z)
    g = sigma * g
    if mu is not None:
        w1 = np.array(mu, dtype=np.float64)
        w1[:n_dyn] = 0.0
        t1 = np.full(ev.n_variables, np.nan)
        ev.eval_constraint_jacobian_transpose_product(t1, Z, w1)
        g = g + t1
    L = ev.dynamics_solve_all(Z, pack_states(p, offset, D, g), adjoint=True)[:, 0]
    w2 = dynamics_rows(p, offset, row0, ev.n_constraints, L)
    t = np.full(ev.n_variables, np.nan)
    ev.eval_constraint_jacobian_transpose_product(t, Z, w2)
    mut = -w2
    if mu is not None:
        mut[n_dyn:] = np.asarray(mu)[n_dyn:]
    else:
        mut[n_dyn:] = 0.0
    return finish(p, offset, g, t, L), L, mut


def compose_product(ev, p, Z, sigma, mu, v, mut=None):
    """y by steps 1 .. 8 of dto_reduced_hessian_product"""
    D, offset, row0 = _layout(ev, p)
    if mut is None:
        mut = compose_gradient(ev, p, Z, sigma, mu)[2]
    N, z = p.N, p.z
    vh = np.array(v, dtype=np.float64)
    vk = vh[:N * z].reshape(N, z)
    v1 = pack_states(p, offset, D, np.where(np.arange(v.size) < z, v, 0.0))[0]      # knot 1 alone: the S entries of v are not read
    for it in p.integrators:
        vk[:, it.x_off:it.x_off + it.x_dim] = 0.0
    rho = np.full(ev.n_constraints, np.nan)
    ev.eval_constraint_jacobian_product(rho, Z, vh)
    B = np.zeros((N, 1, D))
    B[0] = v1
    for i, it in enumerate(p.integrators):
        B[1:, 0, offset[i]:offset[i] + it.x_dim] = -rho[row0[i]:row0[i] + (N - 1) * it.x_dim].reshape(N - 1, it.x_dim)
    Y = ev.dynamics_solve_all(Z, B)[:, 0]
    zh = vh.copy()
    zk = zh[:N * z].reshape(N, z)
    for i, it in enumerate(p.integrators):
        zk[:, it.x_off:it.x_off + it.x_dim] = Y[:, offset[i]:offset[i] + it.x_dim]
    q = np.full(ev.n_variables, np.nan)
    ev.eval_hessian_lagrangian_product(q, Z, zh, sigma, mut)
    G = ev.dynamics_solve_all(Z, pack_states(p, offset, D, q), adjoint=True)[:, 0]
    t = np.full(ev.n_variables, np.nan)
    ev.eval_constraint_jacobian_transpose_product(t, Z, dynamics_rows(p, offset, row0, ev.n_constraints, G))
    return finish(p, offset, q, t, G)
