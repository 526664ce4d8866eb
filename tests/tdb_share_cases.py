"""Problems whose TimeDependentBilinearIntegrators are driven by one system (the groups of DTO_FLAG_SHARED_GENERATORS on the
time-dependent kind), as oracle `Problem`s; reference values through tests/tdb_large_cases.reference.

Components: x_1 .. x_P (dims[i] states each), u[m], v[m] (a second control component), du[m], t, s (a second time component), dt.
Member i is an O.TimeDependentBilinearIntegrator on x_i; `members[i]` overrides what it would share with the others."""
import numpy as np

import dto_oracle as O
import tdb_large_cases as L


def family(n, m, n_mods, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((m + 1, n, n)) / np.sqrt(n / 4.0)
    mods = [("cos", 1.7, 0.5 * rng.standard_normal((m + 1, n, n)) / np.sqrt(n / 4.0)),
            ("sin", 0.6, 0.5 * rng.standard_normal((m + 1, n, n)) / np.sqrt(n / 4.0))][:n_mods]
    # further carriers (wide coefficient tables), drawn after the two above: ("cos" | "sin", 0.25 + 0.4 c), a quarter of the weight
    mods += [(("cos", "sin")[c % 2], 0.25 + 0.4 * c, 0.25 * rng.standard_normal((m + 1, n, n)) / np.sqrt(n / 4.0)) for c in range(2, n_mods)]
    return G, mods


def problem(n, P, m=2, order=1, substeps=2, n_mods=2, N=3, derivative_between=False, members=None, bilinear_first=False,
            derivative=True):
    """`members[i]`: dict with any of G, mods, order, substeps, u (0: u, 1: v), t (0: t, 1: s), dim.  `bilinear_first`: a
    BilinearIntegrator with the family's G on x_1 leads the list (member 0 of the time-dependent kind then sits on x_2).
    `derivative=False`: no DerivativeIntegrator (a handle takes eight integrators: the only way to eight members)."""
    members = [{} for _ in range(P)] if members is None else members
    nx = P + (1 if bilinear_first else 0)
    dims = [n] * nx
    for i, mb in enumerate(members):
        dims[i + (1 if bilinear_first else 0)] = mb.get("dim", n)
    x_offs = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    u0 = int(x_offs[-1])
    z = u0 + 3 * m + 3
    t_offs, dt_idx = (z - 3, z - 2), z - 1
    G, mods = family(n, m, n_mods, seed=100 + n)
    integ = []
    if bilinear_first:
        integ.append(O.BilinearIntegrator(0, n, u0, m, G))
    for i, mb in enumerate(members):
        xi = i + (1 if bilinear_first else 0)
        d = dims[xi]
        Gi, modsi = mb.get("G", G), mb.get("mods", mods)
        if d != n:
            Gi = Gi[:, :d, :d].copy()
            modsi = [(k, w, H[:, :d, :d].copy()) for k, w, H in modsi]
        it = O.TimeDependentBilinearIntegrator(int(x_offs[xi]), d, u0 + m * mb.get("u", 0), m, t_offs[mb.get("t", 0)], Gi, modsi,
                                               mb.get("order", order), mb.get("substeps", substeps)).bind(z, dt_idx)
        integ.append(it)
        if derivative_between and i == 0:
            integ.append(O.DerivativeIntegrator(u0, m, u0 + 2 * m))
    if derivative and not derivative_between:
        integ.append(O.DerivativeIntegrator(u0, m, u0 + 2 * m))
    rng = np.random.default_rng(7 + n + P)
    rows = [rng.standard_normal((u0, N)), 0.4 * rng.standard_normal((2 * m, N)), rng.standard_normal((m, N)),
            np.cumsum(np.full(N, 0.3))[None, :], np.cumsum(np.full(N, 0.2))[None, :], 0.25 + 0.1 * rng.random((1, N))]
    return O.Problem(N=N, z=z, dt_idx=dt_idx, integrators=integ, objectives=[O.QuadraticRegularizer(u0, m, np.ones(m))],
                     Z0=np.vstack(rows).T.reshape(-1).copy())


# (n, P, m, order, substeps, n_mods, derivative_between): the 32-row tile (controls held); a DerivativeIntegrator between
# members; exact tiles, no modulation; two drives at order 1 (p = 6, 21 pairs)
CASES = [(65, 2, 1, 0, 2, 2, False),
         (72, 3, 1, 1, 2, 2, True),
         (128, 2, 2, 1, 2, 0, False),
         (72, 2, 2, 1, 2, 2, False)]


def case(n, P, m, order, substeps, n_mods, derivative_between, N=3):
    return problem(n, P, m=m, order=order, substeps=substeps, n_mods=n_mods, N=N, derivative_between=derivative_between)


def lone(n, m, order, substeps, n_mods, N):
    """One integrator of the family on x_1 (and the DerivativeIntegrator): what k_tdb_mfma runs alone."""
    return problem(n, 1, m=m, order=order, substeps=substeps, n_mods=n_mods, N=N)


# ---- the scratch cap of a group launch, restated from DESIGN 4.22 (host arithmetic; the engine's is tdbm_layout and
# find_time_dependent_share_groups)


def slot_doubles(n, m, order, n_mods, need, P):
    """Scratch slot of a group launch of P members in doubles ("Group size"); need 0 / 1 / 2: defect, Jacobian, Hessian."""
    pad32 = lambda v: (v + 31) // 32 * 32
    np_, p, Q = pad32(n), m + 2 + (m if order else 0), (m + 1) * (1 + n_mods)
    P2 = p * (p + 1) // 2
    C1 = (1, 1 + p, 1 + p + P2)[need]
    Ctot = pad32(P * (pad32(C1) if need == 2 else C1)) + (np_ if need == 1 else 0)
    ucols = 32 * P if need == 2 else P
    total = 4 * np_ * Ctot + np_ * np_ + Q * ucols * np_ + (32 * np_ * P if need == 2 else 0) + (1 + p + P2) * Q
    return total + total % 2


def launch_cap(n, m, order, n_mods, members, hessian):
    """Members per launch: the largest count up to 8 whose slot of every callback the handle has stays within 8 MiB; 1: inactive."""
    cap = 1
    for g in range(2, min(members, 8) + 1):
        if 8 * max(slot_doubles(n, m, order, n_mods, need, g) for need in ((0, 1, 2) if hessian else (0, 1))) > 8 << 20:
            break
        cap = g
    return cap


def reference(prob, key):
    return L.reference(prob, ("share",) + tuple(key))
