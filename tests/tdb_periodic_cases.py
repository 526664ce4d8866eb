"""Period-3 trajectories: the values of a problem with hundreds of knots from a five-knot problem (NumPy only).

The persistent grid of the time-dependent kernels takes a second interval per workgroup only beyond two workgroups per compute
unit -- 513 knots on an MI355X -- where `tdb_large_cases.reference` needs minutes.  What a dynamics interval contributes to g, to
the Jacobian and to the Hessian of the Lagrangian depends on `(z_k, z_{k+1}, mu_k)` alone, and an objective term on its knot, so a
trajectory that repeats three knots repeats three intervals:

    short problem   N = 5, knots [a, b, c, a, b]: any problem's Z0 with knots 3 and 4 overwritten by knots 0 and 1; in mu the rows
                    of interval 3 are the rows of interval 0, for every integrator (`short_mu`)
    long problem    the same components, integrators and objective terms at N_L knots, N_L = 2 (mod 3): knot k is
                    [a, b, c][k mod 3], the rows of mu of interval k are the short problem's of interval k mod 3 (`long_mu`)

Rows are integrator-major, then interval-major.  `tile` builds the long problem's expected vectors from the short problem's
through the two sparse structures:

    g          rows of interval k                    the same integrator's rows of short interval k mod 3
    Jacobian   entry (r, c), r in interval k         short (the row's local index in interval k mod 3, c - k z + (k mod 3) z)
    Hessian    both indices on knot k                short knot 0 for k = 0 (interval 0 alone), 4 for k = N_L - 1 (interval N_L - 2,
                                                     a copy of interval 0 like short interval 3), else 1 + (k - 1) mod 3 (short knots
                                                     1, 2, 3 collect intervals (0, 1), (1, 2), (2, 3 = 0) in this order, as knot k
                                                     collects intervals (k - 1, k))
    Hessian    indices on knots (k, k + 1)           short knots (k mod 3, k mod 3 + 1): interval k alone

Every long entry is a copy of one short entry: no arithmetic, so what is bit-exact in the short vectors stays so.
tests/test_tdb_periodic_reference.py pins the mapping on the oracle alone (exact equality)."""
import dataclasses

import numpy as np


def n_long(cu):
    """Knots of the long problem on `cu` compute units: past two trips of the grid of 2 cu workgroups.  The smallest N >= 4 cu + 4
    with N = 2 (mod 3) is 1028 on 256 compute units; the figure asked for there is 1031 (1030 intervals), one period further, so
    one period is added: 1030 = 2 * 512 + 6 intervals, workgroups 0..5 make three trips and the other 506 two."""
    n = 4 * cu + 4
    return n + (2 - n) % 3 + 3


def short_problem(prob):
    """`prob` (N = 5) with knots 3 and 4 overwritten by knots 0 and 1."""
    assert prob.N == 5 and prob.gd == 0 and not prob.constraints
    Z = prob.Z0.reshape(5, prob.z).copy()
    Z[3:5] = Z[0:2]
    return dataclasses.replace(prob, Z0=Z.reshape(-1))


def long_problem(short, N_L):
    assert short.N == 5 and N_L % 3 == 2 and N_L >= 5
    Z = short.Z0.reshape(5, short.z)[np.arange(N_L) % 3]
    return dataclasses.replace(short, N=N_L, Z0=Z.reshape(-1).copy())


def _dims(prob):
    return [it.x_dim for it in prob.integrators]


def short_mu(short, mu):
    """`mu` of the short problem with every integrator's rows of interval 3 replaced by its rows of interval 0."""
    mu = np.array(mu, dtype=np.float64)
    off = 0
    for d in _dims(short):
        mu[off + 3 * d:off + 4 * d] = mu[off:off + d]
        off += 4 * d
    assert off == mu.size
    return mu


def long_mu(short, mu_s, N_L):
    out, off = [], 0
    for d in _dims(short):
        out.append(mu_s[off:off + 4 * d].reshape(4, d)[np.arange(N_L - 1) % 3].reshape(-1))
        off += 4 * d
    return np.concatenate(out)


def _structure(ev):
    """(N, z, 0-based Jacobian rows, cols, Hessian rows, cols) of an O.OracleEvaluator or a dto_amd.Evaluator."""
    if hasattr(ev, "jacobian_structure1"):
        (jr, jc), (hr, hc) = ev.jacobian_structure1(), ev.hessian_structure1()
        N, z = ev.prob.N, ev.prob.z
    else:
        (jr, jc), (hr, hc) = ev.jacobian_structure(), ev.hessian_lagrangian_structure()
        N, z = ev.trajectory.N, ev.trajectory.dim
    return N, z, np.asarray(jr, np.int64) - 1, np.asarray(jc, np.int64) - 1, np.asarray(hr, np.int64) - 1, np.asarray(hc, np.int64) - 1


def _row_places(jr, jc, n_rows, N, z):
    """Per constraint row: its interval and the first row of its (integrator, interval) run.  A dynamics row of interval k has its
    first stored column at k z; rows are integrator-major, then interval-major, so a run ends where the interval changes."""
    assert np.all(np.diff(jc) >= 0)            # column-major order: a row's first entry has its smallest column
    first = np.full(n_rows, -1, dtype=np.int64)
    first[jr[::-1]] = jc[::-1]                 # (repeated indices: the last assignment stays, which is the row's first entry)
    assert np.all(first >= 0) and np.all(first % z == 0), "a row that is no dynamics row"
    k = first // z
    start = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    assert start.size % (N - 1) == 0 and np.array_equal(k[start], np.tile(np.arange(N - 1), start.size // (N - 1)))
    run = np.cumsum(np.concatenate([[1], (k[1:] != k[:-1]).astype(np.int64)])) - 1     # index of the row's run: integrator * K + k
    return k, run, start


def _lookup(keys_s, keys_l, what):
    order = np.argsort(keys_s, kind="stable")
    pos = np.searchsorted(keys_s, keys_l, sorter=order)
    assert np.all(pos < keys_s.size), what
    idx = order[pos]
    assert np.array_equal(keys_s[idx], keys_l), what
    return idx


def tile(short_ev, long_ev, g_s, j_s, h_s):
    """The long problem's (g, Jacobian values, Hessian values) in `long_ev`'s order from the short problem's in `short_ev`'s."""
    Ns, z, jr_s, jc_s, hr_s, hc_s = _structure(short_ev)
    Nl, zl, jr_l, jc_l, hr_l, hc_l = _structure(long_ev)
    assert Ns == 5 and zl == z and Nl % 3 == 2
    Ks, Kl = Ns - 1, Nl - 1
    nv_s = np.int64(Ns * z)
    n_s, n_l = int(np.asarray(g_s).size), int(jr_l.max()) + 1
    assert int(jr_s.max()) + 1 == n_s and n_l * Ks == n_s * Kl
    # rows: the long row's run (integrator, k) -> the short run (integrator, k mod 3), same local index
    k_s, run_s, start_s = _row_places(jr_s, jc_s, n_s, Ns, z)
    k_l, run_l, start_l = _row_places(jr_l, jc_l, n_l, Nl, z)
    assert start_s.size // Ks == start_l.size // Kl
    rows_l = np.arange(n_l, dtype=np.int64)
    row_map = start_s[(run_l // Kl) * Ks + k_l % 3] + (rows_l - start_l[run_l])
    runs = np.arange(start_l.size)
    assert np.array_equal(np.diff(np.append(start_l, n_l)), np.diff(np.append(start_s, n_s))[runs // Kl * Ks + runs % Kl % 3])
    g = np.asarray(g_s)[row_map]
    # Jacobian
    kj = k_l[jr_l]
    j = np.asarray(j_s)[_lookup(jr_s * nv_s + jc_s, row_map[jr_l] * nv_s + (jc_l - kj * z + (kj % 3) * z), "Jacobian entry")]
    # Hessian
    ka, kb = hr_l // z, hc_l // z
    assert np.all((kb == ka) | (kb == ka + 1))
    diag = np.where(ka == 0, 0, np.where(ka == Nl - 1, 4, 1 + (ka - 1) % 3))
    sa = np.where(kb == ka, diag, ka % 3)
    sb = np.where(kb == ka, diag, ka % 3 + 1)
    h = np.asarray(h_s)[_lookup(hr_s * nv_s + hc_s, (hr_l - ka * z + sa * z) * nv_s + (hc_l - kb * z + sb * z), "Hessian entry")]
    return g, j, h


def knot_diagonal(long_ev):
    """Mask of the long Hessian's entries with both indices on one knot."""
    _, z, _, _, hr, hc = _structure(long_ev)
    return hr // z == hc // z
