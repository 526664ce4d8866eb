"""Test helpers: convert an oracle `Problem` (oracle/dto_oracle.py) into the engine's host mirror."""
import numpy as np

import dto_amd
import dto_oracle as O


def to_engine(prob: O.Problem, closure_derivatives="numeric", tdb_on_device=True):
    """Build NamedTrajectory + DirectTrajOptProblem (host mirror) describing the same problem."""
    N, z = prob.N, prob.z
    data = prob.Z0[:z * N].reshape(N, z).T
    # one trajectory component per distinct range mentioned by the problem; leftovers become filler
    ranges = {}
    for it in prob.integrators:
        if isinstance(it, O.TimeDependentBilinearIntegrator):
            ranges[(it.x_off, it.x_dim)] = None
            if it.u_dim:
                ranges[(it.u_off, it.u_dim)] = None
            ranges[(it.t_off, 1)] = None     # (t_off == dt_idx: the timestep's own component, named once)
            continue
        if it.kind == "external":
            continue
        ranges[(it.x_off, it.x_dim)] = None
        if it.kind == "bilinear":
            if it.u_dim:
                ranges[(it.u_off, it.u_dim)] = None
        else:
            ranges[(it.xdot_off, it.x_dim)] = None
    for t in prob.objectives:
        if t.kind not in ("mintime", "knot_sqdist", "knot_closure", "knot_lowrank", "global_closure"):
            ranges[(t.comp_off, t.comp_dim)] = None
    ranges[(prob.dt_idx, 1)] = None
    cuts = sorted(ranges)
    comps, pos, names = {}, 0, {}
    for off, d in cuts:
        assert off >= pos, "overlapping component ranges are not representable"
        if off > pos:
            comps[f"_f{pos}"] = data[pos:off]
        names[(off, d)] = f"c{off}"
        comps[f"c{off}"] = data[off:off + d]
        pos = off + d
    if pos < z:
        comps[f"_f{pos}"] = data[pos:z]
    gdata = prob.Z0[z * N:] if prob.gd else None
    traj = dto_amd.NamedTrajectory(comps, timestep=names[(prob.dt_idx, 1)], global_data=gdata)
    assert traj.dim == z
    integ = []
    for it in prob.integrators:
        if isinstance(it, O.TimeDependentBilinearIntegrator):
            # the DEVICE integrator (csrc/dto_tdb.hip) for the same generator family; `tdb_on_device=False` routes the same
            # closure through the host-evaluated merge path instead
            fam = dto_amd.ModulatedGenerators(it.G, it.mods)
            if it.u_dim == 0:
                integ.append(_tdb_without_drives(fam, it, names, traj, tdb_on_device))
                continue
            integ.append(dto_amd.TimeDependentBilinearIntegrator(fam, names[(it.x_off, it.x_dim)], names[(it.u_off, it.u_dim)],
                                                                 names[(it.t_off, 1)], traj, spline_order=it.spline_order,
                                                                 substeps=it.substeps, on_device=tdb_on_device))
            continue
        if it.kind == "external":
            analytic = closure_derivatives == "analytic"
            integ.append(dto_amd.HostIntegrator(it.f, it.x_dim, traj, jac=it.jac if analytic else None,
                                                hess=it.hess if analytic else None))
            continue
        if it.kind == "bilinear":
            if it.u_dim == 0:
                raise NotImplementedError
            integ.append(dto_amd.BilinearIntegrator(it.G, names[(it.x_off, it.x_dim)], names[(it.u_off, it.u_dim)], traj))
        else:
            integ.append(dto_amd.DerivativeIntegrator(names[(it.x_off, it.x_dim)], names[(it.xdot_off, it.x_dim)], traj))
    obj = dto_amd.NullObjective()
    terms = []
    for i, t in enumerate(prob.objectives):
        if t.kind == "quadratic":
            o = dto_amd.QuadraticRegularizer(names[(t.comp_off, t.comp_dim)], traj, t.R, baseline=t.baseline, times=t.times1)
        elif t.kind == "linear":
            o = dto_amd.LinearRegularizer(names[(t.comp_off, t.comp_dim)], traj, t.R, times=t.times1)
        elif t.kind == "knot_sqdist":
            o = dto_amd.KnotPointObjective.__new__(dto_amd.KnotPointObjective)
            o.kind, o.var_names, o.external, o.A = "sqdist", [], False, None
            o.times = np.asarray(t.times1, dtype=np.int64)
            o.comps = np.asarray(t.comps, dtype=np.int32)
            o.Qs = np.asarray(t.Qs, dtype=np.float64)
            o.params = None if t.params is None else np.asarray(t.params, dtype=np.float64)
        elif t.kind == "global_closure":
            analytic = closure_derivatives == "analytic"
            o = dto_amd.GlobalKnotPointObjective.__new__(dto_amd.GlobalKnotPointObjective)
            o.l, o.grad, o.hess = t.l, (t.grad if analytic else None), (t.hess if analytic else None)
            o.var_names, o.global_names = [], []
            o.times = np.asarray(t.times1, dtype=np.int64)
            o.comps = np.asarray(t.comps, dtype=np.int32)
            o.gcomps = np.asarray(t.gcomps, dtype=np.int32)
            o.Qs = np.asarray(t.Qs, dtype=np.float64)
            nl = max(1, o.times.size)
            o.params = [None] * nl if t.params is None else list(t.params)
            if o.times.size == 0:  # GlobalObjective: the global variables alone
                o._listings = (lambda Zk, g, o=o: [g[o.gcomps]])
        elif t.kind == "knot_lowrank":
            o = dto_amd.KnotPointObjective.__new__(dto_amd.KnotPointObjective)
            o.kind, o.var_names, o.external = "lowrank_infidelity", [], False
            o.times = np.asarray(t.times1, dtype=np.int64)
            o.comps = np.asarray(t.comps, dtype=np.int32)
            o.Qs = np.asarray(t.Qs, dtype=np.float64)
            o.params, o.A = None, np.asarray(t.A, dtype=np.float64)
        elif t.kind == "knot_closure":
            # the host mirror differentiates the closure itself (complex step / differences) unless the test
            # asks for the analytic derivatives to be handed through (closure_derivatives="analytic")
            o = dto_amd.KnotPointObjective.__new__(dto_amd.KnotPointObjective)
            o.kind, o.var_names, o.external = t.l, [], True
            analytic = closure_derivatives == "analytic"
            o.l, o.grad, o.hess = t.l, (t.grad if analytic else None), (t.hess if analytic else None)
            o.times = np.asarray(t.times1, dtype=np.int64)
            o.comps = np.asarray(t.comps, dtype=np.int32)
            o.Qs = np.asarray(t.Qs, dtype=np.float64)
            o.params = [None] * o.times.size if t.params is None else list(t.params)
        else:
            o = dto_amd.MinimumTimeObjective(traj, D=t.D)
        terms.append(prob.w(i) * o)
    if terms:
        obj = terms[0]
        for t in terms[1:]:
            obj = obj + t
    cons = []
    for c in prob.constraints:
        # component indices are passed through a synthetic single name when they form one range
        if c.kind == "global_closure":
            analytic = closure_derivatives == "analytic"
            k = dto_amd.NonlinearGlobalConstraint.__new__(dto_amd.NonlinearGlobalConstraint)
            k.g, k.jac, k.hess = c.g, (c.jac if analytic else None), (c.hess if analytic else None)
            k.equality, k.global_names = bool(c.equality), []
            k.gcomps = np.asarray(c.gcomps, dtype=np.int32)
            k.global_dim, k.g_dim, k.dim = k.gcomps.size, c.g_dim, c.g_dim
            cons.append(k)
            continue
        k = dto_amd.NonlinearKnotPointConstraint.__new__(dto_amd.NonlinearKnotPointConstraint)
        if c.kind == "closure":
            analytic = closure_derivatives == "analytic"
            k.kind, k.var_names, k.c, k.equality, k.external = c.g, [], 0.0, bool(c.equality), True
            k.g, k.jac, k.hess = c.g, (c.jac if analytic else None), (c.hess if analytic else None)
            k.times = np.asarray(c.times1, dtype=np.int64)
            k.comps = np.asarray(c.comps, dtype=np.int32)
            k.params = [None] * k.times.size if c.params is None else list(c.params)
            k.g_dim, k.var_dim = c.g_dim, k.comps.size
            k.dim = k.g_dim * k.times.size
            cons.append(k)
            continue
        k.external = False
        k.kind, k.var_names, k.c, k.equality = c.kind, [], float(c.c), bool(c.equality)
        k.times = np.asarray(c.times1, dtype=np.int64)
        k.comps = np.asarray(c.comps, dtype=np.int32)
        k.g_dim, k.var_dim = 1, k.comps.size
        k.dim = k.times.size
        cons.append(k)
    return dto_amd.DirectTrajOptProblem(traj, obj, integ, constraints=cons)


def _tdb_without_drives(fam, it, names, traj, on_device):
    """The host mirror's TimeDependentBilinearIntegrator for a family without drives (the engine's ABI takes 0..7): the mirror's
    constructor wants a control component, a NamedTrajectory has none of dimension 0, so the description is filled in directly."""
    if not on_device:
        raise NotImplementedError
    o = dto_amd.TimeDependentBilinearIntegrator.__new__(dto_amd.TimeDependentBilinearIntegrator)
    o.family, o.G, o.spline_order, o.substeps = fam, fam, int(it.spline_order), int(it.substeps)
    o.x_name, o.u_name, o.t_name = names[(it.x_off, it.x_dim)], None, names[(it.t_off, 1)]
    o.x_off, o.u_off, o.t_off, o.x_dim, o.u_dim = it.x_off, 0, it.t_off, it.x_dim, 0
    o.f = o.jac = o.hess = None
    o.dim, o.var_dim = it.x_dim * (traj.N - 1), 2 * traj.dim
    return o


TOL, TOL_H = 1e-10, 1e-8  # values / Jacobian, Hessian


def rel_err(a, b):
    """max |a-b| / max(1,|b|) elementwise (the tolerance form of SURVEY.md §8c)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def run_all(ev, prob_o, Z, mu, sigma=1.0, hessian=True):
    """All MOI callbacks through the engine (host-pointer C ABI)."""
    out = {}
    out["f"] = ev.eval_objective(Z)
    g = np.full(ev.shard.grad_len, np.nan); ev.eval_objective_gradient(g, Z); out["grad"] = g
    c = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(c, Z); out["cons"] = c
    j = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(j, Z); out["jac"] = j
    if hessian:
        h = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(h, Z, sigma, mu); out["hess"] = h
    return out


def check_callbacks(prob_o, Z=None, seed=0, hessian=True, tag="", closure_derivatives="numeric", tol_h=TOL_H, products=False):
    """Every callback of a fresh engine handle against the oracle on prob_o: sparsity bit-exact, values at TOL / tol_h;
    products: J w and J' w as well."""
    ev_o = O.OracleEvaluator(prob_o)
    ev = dto_amd.Evaluator(to_engine(prob_o, closure_derivatives), eval_hessian=hessian)
    try:
        assert ev.n_variables == prob_o.n_vars
        assert ev.n_constraints == ev_o.n_constraints
        assert ev.n_dynamics_constraints == ev_o.n_dynamics_constraints
        jr, jc = ev.jacobian_structure()
        r1, c1 = ev_o.jacobian_structure1()
        assert np.array_equal(jr, r1) and np.array_equal(jc, c1), "Jacobian structure"
        hr, hc = ev.hessian_lagrangian_structure()
        r1, c1 = ev_o.hessian_structure1()
        assert np.array_equal(hr, r1) and np.array_equal(hc, c1), "Hessian structure"
        lo, hi = ev.constraint_bounds()
        lo_o, hi_o = ev_o.row_bounds()
        assert np.array_equal(lo, lo_o) and np.array_equal(hi, hi_o)
        rng = np.random.default_rng(seed)
        Z = prob_o.Z0.copy() if Z is None else Z
        mu = rng.standard_normal(ev_o.n_constraints)
        out = run_all(ev, prob_o, Z, mu, sigma=0.7, hessian=hessian)
        errs = {
            "f": rel_err(out["f"], ev_o.eval_objective(Z)),
            "grad": rel_err(out["grad"], ev_o.eval_objective_gradient(Z)),
            "cons": rel_err(out["cons"], ev_o.eval_constraint(Z)),
            "jac": rel_err(out["jac"], ev_o.eval_constraint_jacobian(Z)),
        }
        if hessian:
            errs["hess"] = rel_err(out["hess"], ev_o.eval_hessian_lagrangian(Z, 0.7, mu))
        if products:
            w = rng.standard_normal(prob_o.n_vars)
            y = np.full(ev_o.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, Z, w)
            errs["Jw"] = rel_err(y, ev_o.eval_constraint_jacobian_product(Z, w))
            w = rng.standard_normal(ev_o.n_constraints)
            y = np.full(prob_o.n_vars, np.nan); ev.eval_constraint_jacobian_transpose_product(y, Z, w)
            errs["JTw"] = rel_err(y, ev_o.eval_constraint_jacobian_transpose_product(Z, w))
        print(tag, errs, ev.last_stats())
        for k, v in errs.items():
            assert v <= (tol_h if k == "hess" else TOL), (tag, k, v)
    finally:
        ev.close()


# ---- full-size outputs checked through sampled knots: knot k of a long horizon against the two-knot oracle problem (z_k, z_{k+1}) --
# the bilinear and derivative integrators couple nothing else, so block k of the big problem IS block 0 of
# that sub-problem


def sub_problem(G, Zk2, n, m, z, dt_idx, extra_objectives=()):
    """Oracle problem on the two knots (z_k, z_{k+1}) with the big problem's generators and objective terms."""
    return O.Problem(N=2, z=z, dt_idx=dt_idx,
                     integrators=[O.BilinearIntegrator(0, n, n, m, G), O.DerivativeIntegrator(n, m, n + m)],
                     objectives=[O.QuadraticRegularizer(n, m, np.ones(m))] + list(extra_objectives),
                     Z0=np.ascontiguousarray(Zk2).reshape(-1).copy())


def dense(rows1, cols1, vals, shape):
    M = np.zeros(shape)
    M[rows1 - 1, cols1 - 1] = vals
    return M


def jac_column_block(get, k, z, D, K):
    """Rows of column block k of the full-size Jacobian slab as a (cnt x z) array: per column and integrator the rows of
    interval k-1, then of interval k.  `get(lo, hi)` returns a host copy of vals[lo:hi]."""
    cnt = (1 if k >= 1 else 0) + (1 if k < K else 0)
    start = 0 if k == 0 else z * D + (k - 1) * 2 * z * D
    return get(start, start + z * cnt * D).reshape(z, cnt * D).T, cnt


def check_jacobian_block(blk, cnt, k, sub_jac, n, m, z, K):
    """blk: (cnt*D x z) of knot k; sub_jac: dense (D x 2z) Jacobian of interval k from the two-knot oracle problem (rows:
    bilinear n, derivative m).  Own rows = its z_k half; previous interval's rows = the constant z_{k+1} half."""
    has_prev = k >= 1
    if k < K:
        own_b = blk[(n if has_prev else 0):(n if has_prev else 0) + n]
        own_d = blk[cnt * n + (m if has_prev else 0):cnt * n + (m if has_prev else 0) + m]
        assert rel_err(own_b, sub_jac[:n, :z]) <= 1e-10, ("bilinear rows", k, rel_err(own_b, sub_jac[:n, :z]))
        assert rel_err(own_d, sub_jac[n:, :z]) <= 1e-10, ("derivative rows", k)
        assert np.all(own_b[:, n + m:n + 2 * m] == 0.0)  # du columns: structural zeros that are still stored
    if has_prev:
        prev_b, prev_d = blk[:n], blk[cnt * n:cnt * n + m]
        ref_b = np.zeros((n, z)); ref_b[:, :n] = np.eye(n)
        ref_d = np.zeros((m, z)); ref_d[:, n:n + m] = np.eye(m)
        assert np.array_equal(prev_b, ref_b) and np.array_equal(prev_d, ref_d), ("z_{k+1} half", k)


def hess_diag_block(get, k, z):
    """Upper triangle (incl. diagonal) of diagonal block k and the off-diagonal block (k-1, k) of the full-size Hessian."""
    tri = z * (z + 1) // 2
    if k == 0:
        return tri_from_cols(get(0, tri), z), None
    start = tri + (k - 1) * (z * z + tri)
    v = get(start, start + z * z + tri)
    Hd, Ho = np.zeros((z, z)), np.zeros((z, z))
    pos = 0
    for b in range(z):
        Ho[:, b] = v[pos:pos + z]
        pos += z
        Hd[:b + 1, b] = v[pos:pos + b + 1]
        pos += b + 1
    return Hd, Ho


def tri_from_cols(v, z):
    Hd = np.zeros((z, z))
    pos = 0
    for b in range(z):
        Hd[:b + 1, b] = v[pos:pos + b + 1]
        pos += b + 1
    return Hd


def sampled_checks(prob_e, ev, n, m, ks, jac_get=None, hess_get=None, cons=None, mu=None, sigma=1.0, extra_objectives=()):
    """Compare column block / Hessian diagonal block of every sampled knot with the two-knot oracle problem."""
    traj = prob_e.trajectory
    N, z = traj.N, traj.dim
    K, D = N - 1, n + m
    dt_idx = traj.components[traj.timestep][0]
    G = prob_e.integrators[0].G
    X = traj.data
    for k in ks:
        if k < K:
            sub = sub_problem(G, X[:, k:k + 2].T, n, m, z, dt_idx, extra_objectives)
            ev_o = O.OracleEvaluator(sub)
            r1, c1 = ev_o.jacobian_structure1()
            sub_jac = dense(r1, c1, ev_o.eval_constraint_jacobian(sub.Z0), (D, 2 * z))
        if jac_get is not None:
            blk, cnt = jac_column_block(jac_get, k, z, D, K)
            check_jacobian_block(blk, cnt, k, sub_jac if k < K else None, n, m, z, K)
            if k < K and cons is not None:
                # chain vs sweep: the dense -E_k of the propagator chain applied to x_k equals exp(A_k) x_k of the sweep
                own = blk[(n if k >= 1 else 0):(n if k >= 1 else 0) + n]
                delta = cons[k * n:(k + 1) * n]
                assert rel_err(own[:, :n] @ X[:n, k], delta - X[:n, k + 1]) <= 1e-10, ("chain vs sweep", k)
        if cons is not None and k < K:
            ref = ev_o.eval_constraint(sub.Z0)
            assert rel_err(cons[k * n:(k + 1) * n], ref[:n]) <= 1e-10, ("bilinear defect", k)
            assert rel_err(cons[K * n + k * m:K * n + (k + 1) * m], ref[n:]) <= 1e-10, ("derivative defect", k)
        if hess_get is not None:
            Hd, Ho = hess_diag_block(hess_get, k, z)
            if Ho is not None:
                assert np.all(Ho == 0.0), ("off-diagonal block", k)  # these integrators never fill it
            if k < K:
                mu_sub = np.concatenate([mu[k * n:(k + 1) * n], mu[K * n + k * m:K * n + (k + 1) * m]])
                r1, c1 = ev_o.hessian_structure1()
                Hs = dense(r1, c1, ev_o.eval_hessian_lagrangian(sub.Z0, sigma, mu_sub), (2 * z, 2 * z))
                assert rel_err(Hd, Hs[:z, :z]) <= 1e-8, ("diagonal block", k, rel_err(Hd, Hs[:z, :z]))
                assert np.all(Hd[:n, :n] == 0.0)  # (x_k, x_k): identically zero for a defect linear in x
            else:
                # last knot: only the objective term of that knot
                sub = sub_problem(G, X[:, k - 1:k + 1].T, n, m, z, dt_idx, extra_objectives)
                Hs = O.objective_full_hessian(sub, sub.Z0).toarray()[z:, z:]
                assert rel_err(Hd, sigma * np.triu(Hs)) <= 1e-8, ("last knot", k)


def host_getter(vals):
    return lambda lo, hi: vals[lo:hi]


# ---- the form a generator sweep ran in (dto_profile_get "sweep_gs" .. "sweep_step": one count per sweep while profiling is on)
SWEEP_FORMS = ("gs", "fused", "s64", "cluster", "step")


def sweep_forms(ev):
    """Generator sweeps since the last profile_reset, by the form they took."""
    return {f: ev.profile_get("sweep_" + f)[1] for f in SWEEP_FORMS}


def assert_sweep_form(counts, form, zero=None, what=""):
    """`form` ran; none of the forms in `zero` (default: every other form) did."""
    zero = [f for f in SWEEP_FORMS if f != form] if zero is None else zero
    assert counts[form] >= 1 and all(counts[f] == 0 for f in zero), (what, form, counts)
