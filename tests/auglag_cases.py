"""Shared by the tests of the augmented-Lagrangian terms (dto_auglag_*; csrc/dto_auglag_plan.h, csrc/dto_auglag.hip): the row rules
restated in NumPy, the cases (built from reduced_cases and the oracle), the dense reference from the ORACLE alone and the outer loop of
the README around any step and merit.

Dense reference at (Z, sigma, mu, rho), Z dynamically feasible:
    g_c      the non-dynamics rows of the oracle's constraint values;  (psi, mult, weight) = rows_restated(is_eq, g_c, mu_c, rho_c)
    Phi(Z)   sigma f(Zf) + sum psi(g_c(Zf)),  Zf = reduced_cases.oracle_feasible(Z)
    r_AL     reduced_cases' r_ref at mu_eff = [0; mult]
    H_AL     H(Z; sigma, [lam; mult]) + J_c' diag(weight) J_c,   Hr_AL = T' H_AL T
rho = 10 on every non-dynamics row; mu is drawn so that between a quarter and three quarters of the inequality rows are active and no
row has |s| = |mu + rho g| below 1e-3 (asserted in `case`)."""
import copy
import functools

import numpy as np

import dto_oracle as O
import newton_box_cases as B
import reduced_cases as R
from helpers import to_engine
from quadform_cases import sym, with_quadforms

RHO = 10.0
SIGMA = R.SIGMA
CASES = ["al_12x9", "al_8x70", "al_8x300", "tdb_order1", "structured_16x4", "quadform_6x6"]
SMALL_CASES = ["al_12x9", "tdb_order1", "quadform_6x6"]        # what the CPU tests afford with dense matrices
# The cases held to the oracle's VALUES: kappa <= reduced_cases.KAPPA_CAP with H_AL (test_auglag_reference.py).  al_8x70 (kappa 1e4 .. 3.5e4
# for random directions) and al_8x300 (no dense matrix) are held to the bits alone.
VALUE_CASES = ["al_12x9", "tdb_order1", "structured_16x4", "quadform_6x6"]
C_BOUND = 0.05


# ------------------------------------------------------------------------------------------------------ the rules, restated
def rows_restated(is_eq, g, mu, rho):
    """(psi, mult, weight, viol) per row by the rules of csrc/dto_auglag_plan.h, every operation rounded on its own"""
    is_eq = np.asarray(is_eq, dtype=bool)
    g, mu, rho = (np.asarray(a, dtype=np.float64) for a in (g, mu, rho))
    with np.errstate(all="ignore"):
        bad = ~(rho >= 0.0) | np.isnan(g) | np.isnan(mu)
        viol = np.where(np.isnan(g), g, np.where(is_eq, np.abs(g), np.where(g > 0.0, g, 0.0)))
        s = mu + rho * g
        active = is_eq | (s > 0.0)
        psi = np.where(active, (mu + (0.5 * rho) * g) * g, -((mu * mu) / (2.0 * rho)))
        mult = np.where(active, s, 0.0)
        weight = np.where(active, rho, 0.0)
        plain = rho == 0.0
        psi, mult, weight = np.where(plain, mu * g, psi), np.where(plain, mu, mult), np.where(plain, 0.0, weight)
        nan = np.full(g.shape, np.nan)
        psi, mult, weight = np.where(bad, nan, psi), np.where(bad, nan, mult), np.where(bad, nan, weight)
    return psi, mult, weight, viol


def lane_sum(x):
    """k_feas_merit's order: lane l adds x[l], x[l + 64], .. ascending from 0.0, then the halving tree"""
    x = np.asarray(x, dtype=np.float64)
    a = np.zeros(-(-max(x.size, 1) // 64) * 64)
    a[:x.size] = x
    lane = np.zeros(64)
    with np.errstate(all="ignore"):
        for row in a.reshape(-1, 64):
            lane = lane + row
        for off in (32, 16, 8, 4, 2, 1):
            lane = lane[:off] + lane[off:2 * off]
    return float(lane[0])


def nanmax0(x):
    """the maximum from 0 that keeps a NaN"""
    x = np.asarray(x, dtype=np.float64)
    return float("nan") if np.isnan(x).any() else float(max(0.0, x.max())) if x.size else 0.0


def info_restated(is_eq, g, mu, rho):
    """the eight scalars of the row pass"""
    psi, mult, weight, viol = rows_restated(is_eq, g, mu, rho)
    with np.errstate(all="ignore"):
        return np.array([lane_sum(psi), float(np.sum(weight != 0.0)), nanmax0(viol), lane_sum(viol * viol), nanmax0(np.abs(mult - mu)),
                         float(np.sum(np.asarray(rho) != 0.0)), 0.0, 0.0])


# ------------------------------------------------------------------------------------------------------------- the cases
def _drives(p):
    it = p.integrators[1]
    assert isinstance(it, O.DerivativeIntegrator)
    return list(range(it.x_off, it.x_off + it.x_dim))


def problem(name):
    """(oracle problem, engine problem, Evaluator keywords)"""
    if name.startswith("al_"):
        n, N = (int(v) for v in name[3:].split("x"))
        p, kw = R.problem(f"scaled_{n}x{N}+con")
        u = _drives(p)
        p.constraints[0].c = C_BOUND                                          # ||u|| - 0.05 <= 0 at the interior knots: violated at the start
        p.constraints.append(O.KnotConstraint("sqnorm", u, 0.04 ** 2, [N // 2], equality=True))
        if name == "al_12x9":
            p.constraints.append(O.KnotConstraint("norm", u, 0.06, [3, 6, 3], equality=False))       # `times` repeat knot 3
        return p, to_engine(p), kw
    if name in ("tdb_order1", "structured_16x4"):
        p, kw = R.problem(name)
        p.constraints = list(p.constraints) + [O.KnotConstraint("norm", _drives(p), C_BOUND, list(range(2, p.N)), equality=False)]
        return p, to_engine(p), kw
    if name == "quadform_6x6":
        base, kw = R.problem("scaled_6x6+con")
        base.constraints[0].c = C_BOUND
        spec = dict(comps=list(range(6)), times1=[3, 6], M=sym(np.random.default_rng(3), 6), c=0.5, equality=False)
        p, pe, _ = with_quadforms(base, [spec])
        return p, pe, kw
    raise KeyError(name)


def row_flags(p):
    return np.concatenate([np.full(c.g_dim * len(c.times1), bool(c.equality)) for c in p.constraints])


def constraint_values(p, Z):
    return np.concatenate([O.constraint_evaluate(c, p, Z) for c in p.constraints])


def full(n_dyn, rows):
    return np.concatenate([np.zeros(n_dyn), rows])


def draw_mu(is_eq, g, rng):
    """s = mu + RHO g is a draw with |s| in [0.05, 1.05] and alternating signs on the rows: about half of the inequality rows are active"""
    s = (0.05 + rng.random(g.size)) * np.where(np.arange(g.size) % 2 == 0, 1.0, -1.0)
    return np.where(is_eq, rng.standard_normal(g.size), s - RHO * g)


@functools.lru_cache(maxsize=None)
def case(name, dense=True):
    """the problems, the FEASIBLE point, mu and rho (n_cons each), the rows' restatement at the point and (dense) the reference:
    computed once, shared, never written"""
    p, pe, kw = problem(name)
    Z = R.oracle_feasible(p, np.ascontiguousarray(p.Z0, dtype=np.float64))
    n_dyn = sum(it.x_dim for it in p.integrators) * (p.N - 1)
    is_eq = row_flags(p)
    g = constraint_values(p, Z)
    mu_c = draw_mu(is_eq, g, np.random.default_rng(17))
    rho_c = np.full(g.size, RHO)
    psi, mult, weight, viol = rows_restated(is_eq, g, mu_c, rho_c)
    ineq = ~is_eq
    share = float(np.mean(weight[ineq] != 0.0))
    assert 0.25 <= share <= 0.75, (name, share)
    assert np.min(np.abs(mu_c + RHO * g)[ineq]) >= 1e-3
    assert np.mean(g[ineq] > 0.0) > 0.5, "most rows are violated at the start"
    out = dict(p=p, pe=pe, kw=kw, Z=Z, n_dyn=n_dyn, n_cons=n_dyn + g.size, is_eq=is_eq, mu=full(n_dyn, mu_c), rho=full(n_dyn, rho_c),
               mu_eff=full(n_dyn, mult), weight=full(n_dyn, weight), share=share)
    if dense:
        out["ref"] = dense_reference(p, Z, SIGMA, out["mu"], out["rho"])
        out["levels"] = R.plan(R.describe(p), p.dt_idx, p.N - 1)["n_levels"]
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------ the dense reference
def rows_at(p, Z, mu, rho):
    n_dyn = sum(it.x_dim for it in p.integrators) * (p.N - 1)
    mu_c = np.zeros(len(rho) - n_dyn) if mu is None else np.asarray(mu)[n_dyn:]
    return n_dyn, rows_restated(row_flags(p), constraint_values(p, Z), mu_c, np.asarray(rho)[n_dyn:])


def phi_ref(p, Z, sigma, mu, rho, trajectory=False):
    Zf = R.oracle_feasible(p, Z)
    _, (psi, _, _, viol) = rows_at(p, Zf, mu, rho)
    phi = sigma * O.objective_value(p, Zf) + float(np.sum(psi))
    return (phi, Zf, float(np.max(viol))) if trajectory else phi


def dense_reference(p, Z, sigma, mu, rho):
    """reduced_cases.dense_reference at mu_eff with H_AL = H + J_c' W J_c in place of H (nH is ||H_AL||)"""
    n_dyn, (psi, mult, weight, viol) = rows_at(p, Z, mu, rho)
    ref = R.dense_reference(p, Z, sigma, full(n_dyn, mult))
    Jc = R.constraint_rows(p, Z)
    H = ref["H"] + Jc.T @ (weight[:, None] * Jc)
    T = ref["T"]
    return dict(ref, H=H, Hr=T.T @ H @ T, nH=float(np.linalg.norm(H, 2)), mult=mult, weight=weight, max_viol=float(np.max(viol)),
                P=float(np.sum(psi)))


# ------------------------------------------------------------------------------------------------------ the outer loop
# The inner step's settings.  shift = 1 regularises the model: with shift = 0 the indefinite reduced Hessian lets a perturbation of 1e-13
# in the operators change max viol by tens of per cent within two outer iterations and flip decisions in the third (measured with the
# oracle's operators alone, test_auglag_reference.py repeats it); with shift = 1 such a perturbation changes no decision.
STEP_KW = dict(rtol=1e-6, shift=1.0)


def outer_loop(step, merit, rows, Z, n_dyn, n_rows, outer=5, trials=10, rho0=RHO):
    """The README's outer loop: per outer iteration the trust-region loop of newton_box_cases on Phi(.; mu, rho), then mu <- mu_eff and
    rho x 10 where max viol did not fall by a factor of 4.
        step(Z, delta, mu, rho) -> (predicted, status, Zp);  merit(Zp, mu, rho) -> (Phi, Zf);  rows(Z, mu, rho) -> (mu_eff, max viol)
    Returns per outer iteration the accept / reject decisions, whether rho grew and max viol behind it; and the first max viol."""
    mu, rho = np.zeros(n_dyn + n_rows), full(n_dyn, np.full(n_rows, rho0))
    _, viol = rows(Z, mu, rho)
    log = dict(viol0=viol, accepted=[], grew=[], viol=[])
    for _ in range(outer):
        phi, Z = merit(Z, mu, rho)
        iterates, _, accepted = B.trust_region_loop(lambda Zk, delta: step(Zk, delta, mu, rho), lambda Zp: merit(Zp, mu, rho), Z, phi,
                                                    trials=trials)
        Z = iterates[-1]
        mu, new_viol = rows(Z, mu, rho)
        grew = not new_viol <= viol / 4.0
        if grew:
            rho = rho * 10.0
        viol = new_viol
        log["accepted"].append(accepted)
        log["grew"].append(grew)
        log["viol"].append(viol)
    return log


@functools.lru_cache(maxsize=None)
def oracle_outer_run(name="al_12x9", eps=0.0):
    """the outer loop with the oracle's dense operators alone; eps > 0 multiplies every gradient, product and merit value by
    1 + eps N(0, 1) per entry: a stand-in for another implementation's rounding"""
    c = case(name, dense=False)
    p = c["p"]
    nonfixed = B.nonfixed_of(p)
    rng = np.random.default_rng(1)
    noise = lambda size=None: 1.0 + eps * rng.standard_normal(size)

    def step(Z, delta, mu, rho):
        ref = dense_reference(p, Z, SIGMA, mu, rho)
        out = B.box_loop(lambda d: R.product_ref(ref, d) * noise(d.size), ref["r_ref"] * noise(Z.size), nonfixed, Z, radius=delta, **STEP_KW)
        return out["info"][6], int(out["info"][0]), out["Zp"]

    def merit(Zp, mu, rho):
        phi, Zf, _ = phi_ref(p, Zp, SIGMA, mu, rho, trajectory=True)
        return phi * noise(), Zf

    def rows(Z, mu, rho):
        n_dyn, (_, mult, _, viol) = rows_at(p, Z, mu, rho)
        return full(n_dyn, mult), float(np.max(viol))

    return outer_loop(step, merit, rows, c["Z"], c["n_dyn"], c["n_cons"] - c["n_dyn"])


# ----------------------------------------------------------------------------- the composition: today's public methods and NumPy
def gauss_newton_term(ev, Z, weight, zh):
    """t = J' [0; weight .* (J z^) on the non-dynamics rows], by the two public products"""
    n_dyn = ev.n_dynamics_constraints
    c = np.full(ev.n_constraints, np.nan)
    ev.eval_constraint_jacobian_product(c, Z, zh)
    w = np.zeros(ev.n_constraints)
    w[n_dyn:] = np.asarray(weight)[n_dyn:] * c[n_dyn:]
    t = np.full(ev.n_variables, np.nan)
    ev.eval_constraint_jacobian_transpose_product(t, Z, w)
    return t


def compose_product(ev, p, Z, sigma, mu_eff, weight, v, S=None, mut=None):
    """reduced_cases.compose_product (S = None) or reduced_input_cases.compose_product (S the store) at mu_eff, with the one rounded
    addition q + t between the Hessian product and the gather of q_S"""
    import reduced_input_cases as RI
    D, offset, row0 = R._layout(ev, p)
    if mut is None:
        mut = R.compose_gradient(ev, p, Z, sigma, mu_eff)[2]
    N, z = p.N, p.z
    if S is None:
        vh = np.array(v, dtype=np.float64)
        vk = vh[:N * z].reshape(N, z)
        v1 = R.pack_states(p, offset, D, np.where(np.arange(v.size) < z, v, 0.0))[0]
        for it in p.integrators:
            vk[:, it.x_off:it.x_off + it.x_dim] = 0.0
        rho = np.full(ev.n_constraints, np.nan)
        ev.eval_constraint_jacobian_product(rho, Z, vh)
        Bm = np.zeros((N, 1, D))
        Bm[0] = v1
        for i, it in enumerate(p.integrators):
            Bm[1:, 0, offset[i]:offset[i] + it.x_dim] = -rho[row0[i]:row0[i] + (N - 1) * it.x_dim].reshape(N - 1, it.x_dim)
        zh = vh
    else:
        Bm = RI.forward(p, offset, D, S, v)
        zh = np.array(v, dtype=np.float64)
    Y = ev.dynamics_solve_all(Z, Bm)[:, 0]
    zk = zh[:N * z].reshape(N, z)
    for i, it in enumerate(p.integrators):
        zk[:, it.x_off:it.x_off + it.x_dim] = Y[:, offset[i]:offset[i] + it.x_dim]
    q = np.full(ev.n_variables, np.nan)
    ev.eval_hessian_lagrangian_product(q, Z, zh, sigma, mut)
    q = q + gauss_newton_term(ev, Z, weight, zh)
    G = ev.dynamics_solve_all(Z, R.pack_states(p, offset, D, q), adjoint=True)[:, 0]
    if S is not None:
        return RI.transposed(p, offset, S, q, G)
    t = np.full(ev.n_variables, np.nan)
    ev.eval_constraint_jacobian_transpose_product(t, Z, R.dynamics_rows(p, offset, row0, ev.n_constraints, G))
    return R.finish(p, offset, q, t, G)


# ------------------------------------------------------------------------- the reference without dense matrices (al_8x300)
def sparse_reference(p, Z, sigma, mu, rho):
    """long_cases' sparse pieces at mu_eff with H_AL as a sparse matrix: r_ref, and `product` (v -> T' H_AL T v as an n_vars vector)"""
    import scipy.sparse as sp
    import long_cases as LC
    n_dyn, (_, mult, weight, _) = rows_at(p, Z, mu, rho)
    q = LC.sparse_pieces(p, Z, sigma, full(n_dyn, mult))
    Jc = LC.constraint_rows(p, Z)
    H = LC.sparse_hessian(O.OracleEvaluator(p), Z, sigma, np.concatenate([q["lam"], mult])) + Jc.T @ sp.diags(weight) @ Jc
    r = np.zeros(p.n_vars)
    r[q["C"]] = LC.apply_Tt(q, q["g"])

    def product(v):
        y = np.zeros(p.n_vars)
        y[q["C"]] = LC.apply_Tt(q, H @ LC.apply_T(q, v[q["C"]]))
        return y

    return dict(C=q["C"], S=q["S"], r_ref=r, product=product)


@functools.lru_cache(maxsize=None)
def scenarios(name):
    """newton_box_cases' scenarios for a case, from the oracle alone: the dense reduced Hessian where the case has one
    (shift = 1.5 |lambda_min| + 0.01 lambda_max, p* by a dense solve), else newton_box_cases.long_scenarios' recipe with the sparse
    product (shift = twice the largest |Rayleigh quotient| of eight power iterations, p* by forty CG iterations)"""
    if name != "al_8x300":
        c = case(name)
        ref, Cidx = c["ref"], c["ref"]["C"]
        Hr = 0.5 * (ref["Hr"] + ref["Hr"].T)
        lam = np.linalg.eigvalsh(Hr)
        shift = 1.5 * abs(lam[0]) + 0.01 * lam[-1]
        gC = ref["r_ref"][Cidx]
        pstar = np.linalg.solve(Hr + shift * np.eye(Cidx.size), -gC)
        return dict(B.scenarios_from(c["Z"], Cidx, gC, shift, pstar), lam=lam, shift=shift, pstar=pstar)
    c = case(name, dense=False)
    ref = sparse_reference(c["p"], c["Z"], SIGMA, c["mu"], c["rho"])
    prod, Cidx, Z = ref["product"], ref["C"], c["Z"]
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
    return dict(B.scenarios_from(Z, Cidx, g[Cidx], shift, x[Cidx]), shift=shift, pstar=x[Cidx])
