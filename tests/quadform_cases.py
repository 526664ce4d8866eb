"""Shared by the quadratic-form knot-constraint tests (DTO_CONSTRAINT_QUADFORM_MINUS_C): the oracle states the term as a
ClosureKnotConstraint with the analytic g = v'Mv - c, jac = 2 (M v)', hess = 2 mu M; the engine-side problem is built directly
(helpers.to_engine serves everything else of the problem)."""
import copy

import numpy as np

import dto_amd
import dto_oracle as O
from helpers import TOL, TOL_H, rel_err, run_all, to_engine


def sym(rng, n, scale=1.0):
    M = rng.standard_normal((n, n)) * scale
    return 0.5 * (M + M.T)


def oracle_quadform(comps, times1, M, c, equality=False):
    M = np.array(M, dtype=np.float64)
    return O.ClosureKnotConstraint(g=lambda v, p: np.array([v @ (M @ v) - c]), jac=lambda v, p: (2.0 * (M @ v))[None, :],
                                   hess=lambda v, p, mu: 2.0 * mu[0] * M, comps=list(comps), times1=list(times1), g_dim=1,
                                   equality=equality)


def engine_quadform(comps, times1, M, c, equality=False):
    k = dto_amd.NonlinearKnotPointConstraint.__new__(dto_amd.NonlinearKnotPointConstraint)
    k.external, k.kind, k.var_names = False, "quadform", []
    k.c, k.equality = float(c), bool(equality)
    k.times = np.asarray(times1, dtype=np.int64)
    k.comps = np.asarray(comps, dtype=np.int32)
    k.M = np.array(M, dtype=np.float64)
    k.g_dim, k.var_dim, k.dim = 1, k.comps.size, k.times.size
    return k


def with_quadforms(base_o, specs):
    """(oracle problem, engine problem with the built-in kind, engine problem with the same terms as host closures with analytic
    derivatives); specs: dicts comps / times1 / M / c / equality, appended behind the base problem's constraints."""
    prob_o = copy.copy(base_o)
    prob_o.constraints = list(base_o.constraints) + [oracle_quadform(**s) for s in specs]
    prob_e = to_engine(base_o)
    prob_e.constraints = list(prob_e.constraints) + [engine_quadform(**s) for s in specs]
    return prob_o, prob_e, to_engine(prob_o, closure_derivatives="analytic")


def to_oracle(prob):
    """The oracle's statement of a host-mirror problem made of the kinds synthetic.unitary_problem and
    synthetic.unitary_minimum_time_problem use."""
    traj = prob.trajectory
    integ = []
    for it in prob.integrators:
        if isinstance(it, dto_amd.BilinearIntegrator):
            integ.append(O.BilinearIntegrator(it.x_off, it.x_dim, it.u_off, it.u_dim, np.asarray(it.G)))
        else:
            integ.append(O.DerivativeIntegrator(it.x_off, it.x_dim, it.xdot_off))
    terms, weights = [], []
    for o, w in zip(prob.objective.objectives, prob.objective.weights):
        if isinstance(o, dto_amd.QuadraticRegularizer):
            terms.append(O.QuadraticRegularizer(o.comp_off, o.comp_dim, np.asarray(o.R)))
        elif isinstance(o, dto_amd.MinimumTimeObjective):
            terms.append(O.MinimumTimeObjective(o.D))
        else:
            terms.append(O.LowRankInfidelityObjective(list(o.comps), list(o.times), list(o.Qs), o.A))
        weights.append(w)
    cons = []
    for c in prob.constraints:
        if c.kind == "quadform":
            cons.append(oracle_quadform(list(c.comps), list(c.times), c.M, c.c, c.equality))
        else:
            cons.append(O.KnotConstraint(c.kind, list(c.comps), c.c, list(c.times), c.equality))
    return O.Problem(N=traj.N, z=traj.dim, dt_idx=traj.components[traj.timestep][0], integrators=integ, objectives=terms,
                     weights=weights, constraints=cons, Z0=np.ascontiguousarray(traj.vec(), dtype=np.float64))


def check_structure(ev, ev_o):
    jr, jc = ev.jacobian_structure()
    r1, c1 = ev_o.jacobian_structure1()
    assert np.array_equal(jr, r1) and np.array_equal(jc, c1), "Jacobian structure"
    hr, hc = ev.hessian_lagrangian_structure()
    r1, c1 = ev_o.hessian_structure1()
    assert np.array_equal(hr, r1) and np.array_equal(hc, c1), "Hessian structure"
    lo, hi = ev.constraint_bounds()
    lo_o, hi_o = ev_o.row_bounds()
    assert np.array_equal(lo, lo_o) and np.array_equal(hi, hi_o), "row bounds"


def check_against_oracle(ev, ev_o, prob_o, Z=None, seed=0, tag=""):
    """Structure bit for bit; f, grad f, g, J, J w, J' w at TOL; H and H v at TOL_H.  Returns the engine's outputs and mu."""
    check_structure(ev, ev_o)
    rng = np.random.default_rng(seed)
    Z = prob_o.Z0.copy() if Z is None else Z
    mu = rng.standard_normal(ev_o.n_constraints)
    out = run_all(ev, prob_o, Z, mu, sigma=0.7, hessian=True)
    figures = {"f": rel_err(out["f"], ev_o.eval_objective(Z)), "grad": rel_err(out["grad"], ev_o.eval_objective_gradient(Z)),
               "cons": rel_err(out["cons"], ev_o.eval_constraint(Z)), "jac": rel_err(out["jac"], ev_o.eval_constraint_jacobian(Z))}
    w = rng.standard_normal(prob_o.n_vars)
    y = np.full(ev_o.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, Z, w)
    figures["Jw"] = rel_err(y, ev_o.eval_constraint_jacobian_product(Z, w))
    wt = rng.standard_normal(ev_o.n_constraints)
    y = np.full(prob_o.n_vars, np.nan); ev.eval_constraint_jacobian_transpose_product(y, Z, wt)
    figures["JTw"] = rel_err(y, ev_o.eval_constraint_jacobian_transpose_product(Z, wt))
    Href = ev_o.eval_hessian_lagrangian(Z, 0.7, mu)
    figures["hess"] = rel_err(out["hess"], Href)
    hv = np.full(prob_o.n_vars, np.nan); ev.eval_hessian_lagrangian_product(hv, Z, w, 0.7, mu)
    r1, c1 = ev_o.hessian_structure1()
    ref = np.zeros(prob_o.n_vars)
    np.add.at(ref, r1 - 1, Href * w[c1 - 1])
    off = r1 != c1
    np.add.at(ref, c1[off] - 1, Href[off] * w[r1[off] - 1])
    figures["Hv"] = rel_err(hv, ref)
    print(tag, figures)
    for k, v in figures.items():
        assert v <= (TOL_H if k in ("hess", "Hv") else TOL), (tag, k, v)
    return out, mu
