"""CPU: tests/tdb_periodic_cases.tile on the oracle alone -- the long problem's g, Jacobian and Hessian of the Lagrangian are the
short problem's entries, copied (exact equality: both sides are the same NumPy arithmetic on the same numbers)."""
import numpy as np

import dto_oracle as O
import tdb_large_cases as L
import tdb_periodic_cases as PC
import tdb_share_cases as S


def _both(short, N_L, sigma=0.6):
    long = PC.long_problem(short, N_L)
    ev_s, ev_l = O.OracleEvaluator(short), O.OracleEvaluator(long)
    mu_s = PC.short_mu(short, np.random.default_rng(1).standard_normal(ev_s.n_constraints))
    mu_l = PC.long_mu(short, mu_s, N_L)
    assert mu_l.size == ev_l.n_constraints
    out = []
    for ev, p, mu in ((ev_s, short, mu_s), (ev_l, long, mu_l)):
        out.append((ev.eval_constraint(p.Z0), ev.eval_constraint_jacobian(p.Z0), ev.eval_hessian_lagrangian(p.Z0, sigma, mu)))
    return ev_s, ev_l, out[0], out[1]


def test_tile_of_the_short_oracle_is_the_long_oracle(N_L=11):
    """8 states, two kets with a DerivativeIntegrator between them, order 1, 11 knots, through the oracle's own integrator."""
    short = PC.short_problem(S.problem(8, 2, m=1, order=1, N=5, derivative_between=True))
    ev_s, ev_l, vs, vl = _both(short, N_L)
    for name, a, b in zip("gJH", PC.tile(ev_s, ev_l, *vs), vl):
        assert a.shape == b.shape and np.array_equal(a, b), (name, float(np.max(np.abs(a - b))))
    assert np.count_nonzero(vl[2]) > 0 and int(PC.knot_diagonal(ev_l).sum()) == N_L * (short.z * (short.z + 1) // 2)


def test_tile_holds_for_the_fast_reference_form_at_one_ket():
    """The form tests/tdb_large_cases.reference uses from 65 states on (here 12 states, order 0, the integrator last in the list)."""
    short = L.fast_problem(PC.short_problem(S.problem(12, 1, m=2, order=0, N=5)))
    for N_L in (5, 8, 14):   # 5: the short problem itself
        ev_s, ev_l, vs, vl = _both(short, N_L)
        for name, a, b in zip("gJH", PC.tile(ev_s, ev_l, *vs), vl):
            assert a.shape == b.shape and np.array_equal(a, b), (N_L, name, float(np.max(np.abs(a - b))))


def test_helpers():
    assert PC.n_long(256) == 1031 and all(PC.n_long(c) % 3 == 2 and 3 <= PC.n_long(c) - 4 * c - 4 < 6 for c in range(1, 400))
    short = PC.short_problem(S.problem(8, 2, m=1, N=5))
    Z = short.Z0.reshape(5, -1)
    assert np.array_equal(Z[3], Z[0]) and np.array_equal(Z[4], Z[1])
    Zl = PC.long_problem(short, 8).Z0.reshape(8, -1)
    assert all(np.array_equal(Zl[k], Z[k % 3]) for k in range(8))
    mu = PC.short_mu(short, np.arange(4.0 * (8 + 8 + 1)))
    assert np.array_equal(mu[24:32], mu[0:8]) and np.array_equal(mu[32 + 24:64], mu[32:40]) and mu[67] == mu[64]
    ml = PC.long_mu(short, mu, 8)
    assert ml.size == 7 * 17 and np.array_equal(ml[3 * 8:4 * 8], mu[0:8]) and np.array_equal(ml[56 + 8 * 4:56 + 8 * 5], mu[32 + 8:32 + 16])
