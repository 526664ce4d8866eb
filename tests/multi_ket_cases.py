"""Shared by the tests of DTO_FLAG_SHARED_GENERATORS: the oracle's statement of synthetic.multi_ket_problem and the positions of
the -E_k blocks of one integrator in the Jacobian's value vector."""
import numpy as np

import dto_amd
import dto_oracle as O


def to_oracle(prob):
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
        else:
            terms.append(O.KnotSqDistObjective(list(o.comps), list(o.times), list(o.Qs), None if o.params is None else np.asarray(o.params)))
        weights.append(w)
    cons = [O.KnotConstraint(c.kind, list(c.comps), c.c, list(c.times), c.equality) for c in prob.constraints]
    return O.Problem(N=traj.N, z=traj.dim, dt_idx=traj.components[traj.timestep][0], integrators=integ, objectives=terms,
                     weights=weights, constraints=cons, Z0=np.ascontiguousarray(traj.vec(), dtype=np.float64))


def multi_ket(n, kets, N, drives=2, seed=3, **kw):
    """multi_ket_problem with the knot constraint on u that interleaves the column offsets"""
    return dto_amd.synthetic.multi_ket_problem(n, kets, drives, N, seed=seed, u_bound=4.0, **kw)


def e_block_index(prob, ev, i):
    """Indices into the (unsharded) Jacobian value vector of the -E_k blocks of integrator i (list position), ordered by
    interval, column, row -- the same order for every integrator of one size."""
    traj = prob.trajectory
    K, z = traj.N - 1, traj.dim
    it = prob.integrators[i]
    n = it.x_dim
    R = K * sum(p.x_dim for p in prob.integrators[:i])
    rows, cols = ev.jacobian_structure()
    r0, c0 = rows - 1 - R, cols - 1
    k = c0 // z
    comp = c0 - k * z
    mask = (r0 >= 0) & (r0 < K * n) & (comp >= it.x_off) & (comp < it.x_off + n) & (r0 // max(n, 1) == k)
    idx = np.nonzero(mask)[0]
    assert idx.size == K * n * n
    return idx
