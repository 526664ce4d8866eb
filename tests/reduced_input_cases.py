"""Shared by the tests of the reduced-space operators' input-block store (option "reduced_input_store"; csrc/dto_input_plan.h,
csrc/dto_reduced.hip): a NumPy restatement of the plan, of the store cut out of an Evaluator's public Jacobian values, and of the two
products in the summation orders the header states -- so that the engine's bits can be reproduced -- and the store route's
composition: reduced_cases.compose_gradient / compose_product with the two Jacobian products replaced by them."""
import numpy as np

import reduced_cases as R
from elim_cases import describe, engine_jacobian_dense

OPTION = "reduced_input_store"
N2_CASE = "scaled_12x2"     # two knots: every knot has one adjacent interval on one side only


def free_inputs(p):
    """per integrator the ascending list fin_a of its free inputs; per knot component its terms [(a, j)] in list order"""
    its = describe(p)
    state = set()
    for i in its:
        state |= set(range(i["x_off"], i["x_off"] + i["x_dim"]))
    fin = []
    for a in its:
        s = set(range(a["in_off"], a["in_off"] + a["in_dim"])) | {p.dt_idx}
        if a["kind"] == "time_dependent":
            s.add(a["t_off"])
        fin.append(sorted(c for c in s if c not in state))
    terms = [[(a, f.index(c)) for a, f in enumerate(fin) if c in f] for c in range(p.z)]
    return fin, terms


def store_from_jacobian(ev, p, Z):
    """F_a (K, 2, Wf_a, x_dim_a) per integrator, cut out of the Evaluator's eval_constraint_jacobian values"""
    J = engine_jacobian_dense(ev, Z)
    fin, terms = free_inputs(p)
    K, F, pre = p.N - 1, [], 0
    for a, it in enumerate(p.integrators):
        Fa = np.zeros((K, 2, len(fin[a]), it.x_dim))
        for k in range(K):
            rows = K * pre + k * it.x_dim + np.arange(it.x_dim)
            for half in (0, 1):
                for j, c in enumerate(fin[a]):
                    Fa[k, half, j] = J[rows, (k + half) * p.z + c]
        F.append(Fa)
        pre += it.x_dim
    return dict(F=F, fin=fin, terms=terms)


def forward(p, offset, D, S, v):
    """B (N, 1, D): the knot-1 states of v, then minus the input blocks times the free inputs of v -- half 0 before half 1, j ascending"""
    N, z = p.N, p.z
    B = np.zeros((N, 1, D))
    B[0] = R.pack_states(p, offset, D, np.where(np.arange(v.size) < z, v, 0.0))[0]
    for a, it in enumerate(p.integrators):
        for k in range(1, N):
            acc = np.zeros(it.x_dim)
            for half in (0, 1):
                for j, c in enumerate(S["fin"][a]):
                    acc = acc + S["F"][a][k - 1, half, j] * v[(k - 1 + half) * z + c]
            B[k, 0, offset[a]:offset[a] + it.x_dim] = -acc
    return B


def transposed(p, offset, S, q, G):
    """y (n_vars): q - t on the read components, one 64-lane accumulation and halving tree per output; q - 0.0 on the unread ones and the
    globals; Gam_0 on the states of knot 0; 0 on the dependent entries"""
    N, z, K = p.N, p.z, p.N - 1
    y = q - 0.0
    yk = y[:N * z].reshape(N, z)
    for kn in range(N):
        for c in range(z):
            if not S["terms"][c]:
                continue
            lanes = np.zeros(64)
            for a, j in S["terms"][c]:
                n = p.integrators[a].x_dim
                for half in (1, 0):
                    iv = kn - 1 if half == 1 else kn
                    if iv < 0 or iv >= K:
                        continue
                    prod = S["F"][a][iv, half, j] * G[iv + 1, offset[a]:offset[a] + n]
                    for s in range(0, n, 64):
                        seg = prod[s:s + 64]
                        lanes[:seg.size] = lanes[:seg.size] + seg
            for off in (32, 16, 8, 4, 2, 1):
                lanes[:off] = lanes[:off] + lanes[off:2 * off]
            yk[kn, c] = q[kn * z + c] - lanes[0]
    for i, it in enumerate(p.integrators):
        yk[:, it.x_off:it.x_off + it.x_dim] = 0.0
        yk[0, it.x_off:it.x_off + it.x_dim] = G[0, offset[i]:offset[i] + it.x_dim]
    return y


def compose_gradient(ev, p, Z, sigma, mu, S):
    """(r, Lam (N, D), mu~): reduced_cases.compose_gradient with t = J' w2 taken from the store"""
    D, offset, row0 = R._layout(ev, p)
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
    L = ev.dynamics_solve_all(Z, R.pack_states(p, offset, D, g), adjoint=True)[:, 0]
    mut = -R.dynamics_rows(p, offset, row0, ev.n_constraints, L)
    mut[n_dyn:] = np.asarray(mu)[n_dyn:] if mu is not None else 0.0
    return transposed(p, offset, S, g, L), L, mut


def compose_product(ev, p, Z, sigma, mu, v, S, mut):
    """y: reduced_cases.compose_product with rho = J v^ and t = J' w taken from the store"""
    D, offset, _ = R._layout(ev, p)
    N, z = p.N, p.z
    Y = ev.dynamics_solve_all(Z, forward(p, offset, D, S, v))[:, 0]
    zh = np.array(v, dtype=np.float64)
    zk = zh[:N * z].reshape(N, z)
    for i, it in enumerate(p.integrators):
        zk[:, it.x_off:it.x_off + it.x_dim] = Y[:, offset[i]:offset[i] + it.x_dim]
    q = np.full(ev.n_variables, np.nan)
    ev.eval_hessian_lagrangian_product(q, Z, zh, sigma, mut)
    G = ev.dynamics_solve_all(Z, R.pack_states(p, offset, D, q), adjoint=True)[:, 0]
    return transposed(p, offset, S, q, G)
