"""Oracle problems for the TimeDependentBilinearIntegrator with replicated-block generators (NumPy only): the pattern of
`O.make_tdb_problem` -- components x, u, (du,) t, dt, QuadraticRegularizer(u) -- with G_j = kron(I_r, B_j) for random b x b blocks
and the carrier matrices likewise.  Reference values come from tests/tdb_large_cases.reference, which is dense and knows nothing
of the structure."""
import numpy as np

import dto_oracle as O


def kron_family(b, r, m, n_mods, rng):
    """(G, mods) of m + 1 generators and n_mods carrier terms (cos 1.7 t, sin 0.6 t), every matrix kron(I_r, B)."""
    s = 1.0 / np.sqrt(b / 4.0)
    rep = lambda B: np.stack([np.kron(np.eye(r), Bj) for Bj in B])
    G = rep(s * rng.standard_normal((m + 1, b, b)))
    mods = [("cos", 1.7, rep(0.5 * s * rng.standard_normal((m + 1, b, b)))),
            ("sin", 0.6, rep(0.5 * s * rng.standard_normal((m + 1, b, b))))][:n_mods]
    return G, mods


def problem_from_family(G, mods, m, order, substeps, N=3, seed=0, with_derivative=False):
    rng = np.random.default_rng(seed)
    n = G.shape[1]
    x = rng.standard_normal((n, N))
    u = 0.4 * rng.standard_normal((m, N))
    t = np.cumsum(np.full(N, 0.3))[None, :]
    dt = 0.25 + 0.1 * rng.random((1, N))
    rows = [x, u]
    z = n + m + 2 + (m if with_derivative else 0)
    if with_derivative:
        rows.append(rng.standard_normal((m, N)))
    rows += [t, dt]
    integ = [O.TimeDependentBilinearIntegrator(0, n, n, m, z - 2, G, mods, order, substeps).bind(z, z - 1)]
    if with_derivative:
        integ.append(O.DerivativeIntegrator(n, m, n + m))
    return O.Problem(N=N, z=z, dt_idx=z - 1, integrators=integ, objectives=[O.QuadraticRegularizer(n, m, np.ones(m))],
                     Z0=np.vstack(rows).T.reshape(-1).copy())


def kron_tdb_problem(b, r, m, order, substeps, n_mods, N=3, with_derivative=False):
    rng = np.random.default_rng(1000 * b + r)
    G, mods = kron_family(b, r, m, n_mods, rng)
    return problem_from_family(G, mods, m, order, substeps, N=N, seed=b + r, with_derivative=with_derivative)
