"""Synthetic benchmark problems of BASELINE.json's configurations.

Shape of the reference's scaling generator ``make_scaled_problem``
(benchmark/problem_utils.jl:49-77): components x[n], u[m], du[m], dt (z = n+2m+1),
[BilinearIntegrator(G,:x,:u), DerivativeIntegrator(:u,:du)], QuadraticRegularizer(:u, 1.0),
G0, G_j ~ randn(n,n), x ~ randn, u ~ 0.1 randn, du ~ randn, dt = 0.1.  Julia's Xoshiro stream is not
reproducible outside Julia, so a counter-based Philox stream (seed 42) is used instead."""
from __future__ import annotations

import numpy as np

from .problem import (BilinearIntegrator, DerivativeIntegrator, DirectTrajOptProblem, KnotPointObjective, LinearRegularizer,
                      MinimumTimeObjective, ModulatedGenerators, NonlinearKnotPointConstraint, QuadraticRegularizer,
                      TimeDependentBilinearIntegrator, fidelity_constraint)
from .trajectory import NamedTrajectory


def scaled_problem_arrays(N, n, m=4, seed=42):
    rng = np.random.Generator(np.random.Philox(seed))
    r = rng.standard_normal((m + 1) * n * n + N * (n + 2 * m))
    G = r[:(m + 1) * n * n].reshape(m + 1, n, n).transpose(0, 2, 1).copy()  # column-major fill order
    rest = r[(m + 1) * n * n:]
    x = rest[:n * N].reshape(N, n).T
    u = 0.1 * rest[n * N:n * N + m * N].reshape(N, m).T
    du = rest[n * N + m * N:].reshape(N, m).T
    return G, x, u, du


def make_scaled_problem(N, n, m=4, seed=42):
    G, x, u, du = scaled_problem_arrays(N, n, m, seed)
    traj = NamedTrajectory({"x": x, "u": u, "du": du, "dt": np.full((1, N), 0.1)}, timestep="dt")
    integrators = [BilinearIntegrator(G, "x", "u", traj), DerivativeIntegrator("u", "du", traj)]
    J = QuadraticRegularizer("u", traj, 1.0)
    return DirectTrajOptProblem(traj, J, integrators)


def make_l1_slack_problem(N, n, m=4, seed=42):
    """BASELINE configs[4] workload on the evaluator path ("C5"): components
    x[n], u[m], du[m], s_du[m], dt (z = n + 3m + 1); [BilinearIntegrator(G,:x,:u), DerivativeIntegrator(:u,:du)];
    NonlinearKnotPointConstraint(u -> [norm(u) - 1], :u, times = 2:N-1, equality = false) as in the reference's
    test/test_snippets.jl:39-45; QuadraticRegularizer(:u, 1.0) + LinearRegularizer(:s_du, 1e-2), the penalty on the slack
    of an L1SlackConstraint (src/constraints/linear/l1_slack_constraint.jl:28 -- its own rows |du| <= s_du are linear and
    are handed to MOI once, they never reach the evaluator)."""
    G, x, u, du = scaled_problem_arrays(N, n, m, seed)
    traj = NamedTrajectory({"x": x, "u": u, "du": du, "s_du": np.abs(du) + 0.1, "dt": np.full((1, N), 0.1)}, timestep="dt")
    integrators = [BilinearIntegrator(G, "x", "u", traj), DerivativeIntegrator("u", "du", traj)]
    J = QuadraticRegularizer("u", traj, 1.0) + LinearRegularizer("s_du", traj, 1e-2)
    con = NonlinearKnotPointConstraint("norm", "u", traj, c=1.0, equality=False, times=range(2, N))
    return DirectTrajOptProblem(traj, J, integrators, constraints=[con])


def unitary_fidelity_factor(goal_iso_cols, levels):
    """A (2 x 2 levels^2) with ||A v||^2 = |tr(U_goal' U)|^2 / levels^2 for v the stacked iso columns [Re u_c; Im u_c]."""
    g = np.asarray(goal_iso_cols, dtype=np.float64).reshape(levels, 2 * levels)
    gr, gi = g[:, :levels], g[:, levels:]
    return np.vstack([np.concatenate([gr, gi], axis=1).reshape(-1), np.concatenate([-gi, gr], axis=1).reshape(-1)]) / levels


def unitary_problem(levels, drives, N, seed=42, dt=0.1, dt_large=None, dt_small=None, a_bound=1.0):
    """A Piccolo-shaped unitary gate-synthesis problem.  Components: U (2 levels^2: the operator in isomorphic coordinates,
    column after column), a (drives), da, dda, dt.  Dynamics G(a) = kron(I_levels, iso(-i H(a))), H(a) = H_0 + sum_j a_j H_j with
    random Hermitian drift and drives -- what ``Evaluator(..., block_generators=True)`` recognises as ``levels`` replicas of a
    2 levels x 2 levels block -- and two DerivativeIntegrators (a, da), (da, dda); QuadraticRegularizers on a, da, dda; a
    terminal unitary-infidelity objective; the knot constraint ||a||^2 - a_bound <= 0 at the interior knots.
    ``dt_large`` / ``dt_small`` replace the timestep of knot 2 / knot 3 (a step whose exponential needs scaling, one that needs
    nothing beyond a few terms)."""
    rng = np.random.Generator(np.random.Philox(seed))
    b, n = 2 * levels, 2 * levels * levels

    def iso_minus_i(H):  # iso(-i H) = [[Im H, Re H], [-Re H, Im H]]
        return np.block([[H.imag, H.real], [-H.real, H.imag]])

    blocks = []
    for _ in range(drives + 1):
        M = rng.standard_normal((levels, levels)) + 1j * rng.standard_normal((levels, levels))
        H = (M + M.conj().T) / (2.0 * np.sqrt(levels))
        blocks.append(iso_minus_i(H))
    G = np.stack([np.kron(np.eye(levels), B) for B in blocks])
    U = rng.standard_normal((n, N)) / np.sqrt(levels)
    a = 0.1 * rng.standard_normal((drives, N))
    da = rng.standard_normal((drives, N))
    dda = rng.standard_normal((drives, N))
    dts = np.full((1, N), float(dt))
    if dt_large is not None and N >= 3:
        dts[0, 1] = dt_large
    if dt_small is not None and N >= 4:
        dts[0, 2] = dt_small
    traj = NamedTrajectory({"U": U, "a": a, "da": da, "dda": dda, "dt": dts}, timestep="dt")
    integrators = [BilinearIntegrator(G, "U", "a", traj), DerivativeIntegrator("a", "da", traj),
                   DerivativeIntegrator("da", "dda", traj)]
    goal = np.linalg.qr(rng.standard_normal((levels, levels)) + 1j * rng.standard_normal((levels, levels)))[0]
    goal_iso = np.concatenate([goal.real, goal.imag], axis=0).T  # row c: [Re u_c; Im u_c]
    A = unitary_fidelity_factor(goal_iso, levels)
    J = (QuadraticRegularizer("a", traj, 1e-2) + QuadraticRegularizer("da", traj, 1e-2) + QuadraticRegularizer("dda", traj, 1e-2)
         + KnotPointObjective("lowrank_infidelity", "U", traj, times=[N], Qs=[100.0], A=A))
    con = NonlinearKnotPointConstraint("sqnorm", "a", traj, c=a_bound, equality=False, times=range(2, N))
    return DirectTrajOptProblem(traj, J, integrators, constraints=[con])


def unitary_tdb_problem(levels, drives, N, n_mods=2, spline_order=1, substeps=16, seed=42, dt=0.1):
    """``unitary_problem`` in the lab frame: its components plus a time component ``t`` (U, a, da, dda, t, dt), and the dynamics a
    TimeDependentBilinearIntegrator on ``ModulatedGenerators`` with G_j = kron(I_levels, iso(-i H_j)) and ``n_mods`` carrier terms
    (cos 1.7 t, sin 0.6 t) H_cj of the same shape, random Hermitian H -- what ``Evaluator(..., block_generators=True)`` recognises
    as ``levels`` replicas of a 2 levels x 2 levels block on the time-dependent path.  The two DerivativeIntegrators (a, da),
    (da, dda), QuadraticRegularizers on a, da, dda and the terminal unitary-infidelity objective are ``unitary_problem``'s."""
    rng = np.random.Generator(np.random.Philox(seed))
    n = 2 * levels * levels

    def family(scale):  # (drives + 1) generators kron(I_levels, iso(-i H)), iso(-i H) = [[Im H, Re H], [-Re H, Im H]]
        out = []
        for _ in range(drives + 1):
            M = rng.standard_normal((levels, levels)) + 1j * rng.standard_normal((levels, levels))
            H = scale * (M + M.conj().T) / (2.0 * np.sqrt(levels))
            out.append(np.kron(np.eye(levels), np.block([[H.imag, H.real], [-H.real, H.imag]])))
        return np.stack(out)

    G = family(1.0)
    mods = [("cos", 1.7, family(0.5)), ("sin", 0.6, family(0.5))][:n_mods]
    U = rng.standard_normal((n, N)) / np.sqrt(levels)
    a = 0.1 * rng.standard_normal((drives, N))
    da = rng.standard_normal((drives, N))
    dda = rng.standard_normal((drives, N))
    dts = np.full((1, N), float(dt))
    t = np.concatenate([[0.0], np.cumsum(dts[0])[:-1]])[None, :]
    traj = NamedTrajectory({"U": U, "a": a, "da": da, "dda": dda, "t": t, "dt": dts}, timestep="dt")
    integrators = [TimeDependentBilinearIntegrator(ModulatedGenerators(G, mods), "U", "a", "t", traj, spline_order=spline_order,
                                                   substeps=substeps),
                   DerivativeIntegrator("a", "da", traj), DerivativeIntegrator("da", "dda", traj)]
    goal = np.linalg.qr(rng.standard_normal((levels, levels)) + 1j * rng.standard_normal((levels, levels)))[0]
    goal_iso = np.concatenate([goal.real, goal.imag], axis=0).T
    A = unitary_fidelity_factor(goal_iso, levels)
    J = (QuadraticRegularizer("a", traj, 1e-2) + QuadraticRegularizer("da", traj, 1e-2) + QuadraticRegularizer("dda", traj, 1e-2)
         + KnotPointObjective("lowrank_infidelity", "U", traj, times=[N], Qs=[100.0], A=A))
    return DirectTrajOptProblem(traj, J, integrators)


def unitary_minimum_time_problem(levels, drives, N, fidelity=0.99, seed=42, D=1.0, closure=False, **kw):
    """The second stage of gate synthesis on ``unitary_problem``'s trajectory, generators and goal (same random stream):
    MinimumTimeObjective(D) plus the three regularizers, the bound ||a||^2 <= a_bound at the interior knots and the
    final-fidelity bound F(U_N) >= fidelity at the last knot, F(v) = ||A v||^2 the unitary fidelity -- the built-in quadratic
    form M = -A'A, c = -fidelity (``fidelity_constraint``).  ``closure=True`` states the same bound as a host closure with
    analytic derivatives (DTO_CONSTRAINT_EXTERNAL: the route such a bound had to take before the built-in kind)."""
    base = unitary_problem(levels, drives, N, seed=seed, **kw)
    traj = base.trajectory
    terms = [(o, w) for o, w in zip(base.objective.objectives, base.objective.weights) if isinstance(o, QuadraticRegularizer)]
    infid = [o for o in base.objective.objectives if isinstance(o, KnotPointObjective)][0]
    J = MinimumTimeObjective(traj, D=D)
    for o, w in terms:
        J = J + w * o
    bound = fidelity_constraint(infid.A, "U", traj, fidelity)
    if closure:
        M, c = bound.M, bound.c
        bound = NonlinearKnotPointConstraint(lambda v, p: np.array([v @ (M @ v) - c]), "U", traj, equality=False, times=[N],
                                             jac=lambda v, p: (2.0 * (M @ v))[None, :], hess=lambda v, p, mu: 2.0 * mu[0] * M)
    return DirectTrajOptProblem(traj, J, base.integrators, constraints=list(base.constraints) + [bound])


def multi_ket_problem(n, kets, drives, N, seed=42, dt=0.1, u_bound=None, extra_ket=False, derivative_between=False, scale=None):
    """A multi-state transfer problem: ``kets`` states driven by ONE system.  Components psi1..psiP (n each), u (drives), du, dt;
    one skew-symmetric drift and ``drives`` skew-symmetric drive generators (a real isomorphic Schroedinger generator, scaled so
    that ||dt G(u)|| stays of order one at any n) shared by P BilinearIntegrators -- what ``Evaluator(..., shared_generators=True)``
    groups -- plus DerivativeIntegrator(u, du); QuadraticRegularizers on u and du and a terminal ||psi_i - goal_i||^2 per ket.
    ``u_bound``: the knot constraint ||u||^2 - u_bound <= 0 at the interior knots (its entries interleave with the integrators'
    in the u columns).  ``scale``: the generators' entries are N(0, scale^2) before antisymmetrisation (default 1 / sqrt(n); 1.0
    gives the norms of ``make_scaled_problem``, whose propagators need several squarings).  ``extra_ket``: one more ket "phi" with generators of its own.  ``derivative_between``: the derivative
    integrator sits between the first ket's integrator and the others in the list instead of at its end."""
    rng = np.random.Generator(np.random.Philox(seed))
    def generators():
        M = rng.standard_normal((drives + 1, n, n))
        return (M - M.transpose(0, 2, 1)) * ((1.0 / np.sqrt(n) if scale is None else float(scale)) / np.sqrt(2.0))
    G = generators()
    u = 0.1 * rng.standard_normal((drives, N))   # (drawn before the kets: generators and controls do not depend on their number)
    du = rng.standard_normal((drives, N))
    comps = {}
    for i in range(kets):
        v = rng.standard_normal((n, N))
        comps[f"psi{i + 1}"] = v / np.linalg.norm(v, axis=0)
    if extra_ket:
        v = rng.standard_normal((n, N))
        comps["phi"] = v / np.linalg.norm(v, axis=0)
    comps["u"], comps["du"] = u, du
    comps["dt"] = np.full((1, N), float(dt))
    traj = NamedTrajectory(comps, timestep="dt")
    kets_int = [BilinearIntegrator(G, f"psi{i + 1}", "u", traj) for i in range(kets)]
    if extra_ket:
        kets_int.append(BilinearIntegrator(generators(), "phi", "u", traj))
    der = DerivativeIntegrator("u", "du", traj)
    integrators = kets_int[:1] + [der] + kets_int[1:] if derivative_between else kets_int + [der]
    J = QuadraticRegularizer("u", traj, 1e-2) + QuadraticRegularizer("du", traj, 1e-2)
    for name in [k for k in comps if k.startswith("psi") or k == "phi"]:
        goal = rng.standard_normal(n)
        J = J + KnotPointObjective("sqdist", name, traj, times=[N], Qs=[10.0], params=(goal / np.linalg.norm(goal))[None, :])
    cons = []
    if u_bound is not None:
        cons.append(NonlinearKnotPointConstraint("sqnorm", "u", traj, c=float(u_bound), equality=False, times=range(2, N)))
    return DirectTrajOptProblem(traj, J, integrators, constraints=cons)


def multi_ket_modulated_problem(n, kets, drives, N, order=1, substeps=16, n_mods=2, seed=42, dt=0.1, derivative_between=False):
    """``multi_ket_problem`` in the lab frame: ``kets`` states driven by ONE time-dependent system.  Components psi1..psiP (n
    each), u (drives), du, t, dt; skew-symmetric drift and drive generators G_j (scaled as ``multi_ket_problem``'s) and ``n_mods``
    carrier terms (cos 1.7 t, sin 0.6 t) H_cj of the same shape at half the scale, shared by P TimeDependentBilinearIntegrators of
    spline order ``order`` with ``substeps`` RK4 steps -- what ``Evaluator(..., shared_generators=True)`` groups and, at 65..256
    states, evaluates with one propagation per group -- plus DerivativeIntegrator(u, du); QuadraticRegularizers on u and du and a
    terminal ||psi_i - goal_i||^2 per ket.  ``derivative_between``: the derivative integrator sits between the first ket's
    integrator and the others in the list instead of at its end."""
    rng = np.random.Generator(np.random.Philox(seed))
    def generators(scale):
        M = rng.standard_normal((drives + 1, n, n))
        return (M - M.transpose(0, 2, 1)) * (scale / np.sqrt(2.0 * n))
    G = generators(1.0)
    mods = [("cos", 1.7, generators(0.5)), ("sin", 0.6, generators(0.5))][:n_mods]
    comps = {"u": 0.1 * rng.standard_normal((drives, N)), "du": rng.standard_normal((drives, N))}
    kets_c = {}
    for i in range(kets):
        v = rng.standard_normal((n, N))
        kets_c[f"psi{i + 1}"] = v / np.linalg.norm(v, axis=0)
    dts = np.full((1, N), float(dt))
    comps = {**kets_c, **comps, "t": np.concatenate([[0.0], np.cumsum(dts[0])[:-1]])[None, :], "dt": dts}
    traj = NamedTrajectory(comps, timestep="dt")
    fam = ModulatedGenerators(G, mods)
    kets_int = [TimeDependentBilinearIntegrator(fam, name, "u", "t", traj, spline_order=order, substeps=substeps) for name in kets_c]
    der = DerivativeIntegrator("u", "du", traj)
    integrators = kets_int[:1] + [der] + kets_int[1:] if derivative_between else kets_int + [der]
    J = QuadraticRegularizer("u", traj, 1e-2) + QuadraticRegularizer("du", traj, 1e-2)
    for name in kets_c:
        goal = rng.standard_normal(n)
        J = J + KnotPointObjective("sqdist", name, traj, times=[N], Qs=[10.0], params=(goal / np.linalg.norm(goal))[None, :])
    return DirectTrajOptProblem(traj, J, integrators)
