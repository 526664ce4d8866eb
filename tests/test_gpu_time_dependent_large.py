"""GPU: the device TimeDependentBilinearIntegrator at 65..256 states (csrc/dto_tdb_mfma.hip: FP64 MFMA products against
M0 = sum_q c_q B_q, derivative jets applied as scalar combinations of B_q y, a persistent grid).

Reference: tests/tdb_large_cases.py -- `O.OracleEvaluator` with the integrator's blocks in a fast, finite-difference-free form of
the same discrete map; tests/test_tdb_large_reference.py pins it to the oracle at 8 and 24 states.  Bars are those of
tests/test_gpu_time_dependent.py: 1e-10 relative for values and Jacobian, 1e-8 for the Hessian.  Shapes are the smallest at which
the path can go wrong: N = 3 (two intervals), N = 5 where sharded.

These bars compare two fp64 codes; accuracy is held in tests/test_gpu_tdb_accuracy_budget.py, where k_tdb_mfma's 32- and 64-row
tile bodies (72 and 128 states) meet 320-bit fixtures of the discrete map at bars of 7e-15 .. 2e-13 per interval and quantity
class, and where tests/tdb_large_cases.py, the reference used here, is itself measured against those fixtures (at most 1.5e-14)."""
import numpy as np
import pytest

import dto_oracle as O
import tdb_large_cases as L
from helpers import rel_err, to_engine

pytestmark = pytest.mark.gpu

CASES = [(65, 1, 0, 2, 2),    # first size past k_tdb's cap: 31 padded rows, the 32-row tile
         (72, 2, 1, 4, 2),
         (128, 2, 1, 3, 0),   # exact tiles, no modulation
         (200, 1, 0, 2, 2),   # ragged
         (256, 2, 1, 2, 2)]   # the cap


def _problem(n, m, order, substeps, n_mods, N=3, with_derivative=False):
    return O.make_tdb_problem(N=N, n=n, m=m, order=order, seed=40 + n, substeps=substeps, n_mods=n_mods, with_derivative=with_derivative)


def _all(ev, Z, mu, sigma=0.6):
    g = np.empty(ev.shard.cons_len); ev.eval_constraint(g, Z)
    j = np.empty(ev.shard.jac_len); ev.eval_constraint_jacobian(j, Z)
    h = np.empty(ev.shard.hess_len); ev.eval_hessian_lagrangian(h, Z, sigma, mu)
    return g, j, h


@pytest.mark.parametrize("n,m,order,substeps,n_mods", CASES)
def test_device_propagator_matches_the_reference(n, m, order, substeps, n_mods):
    import dto_amd
    po = _problem(n, m, order, substeps, n_mods)
    ev_r, mu, g_r, j_r, h_r = L.reference(po, ("parity", n, m, order, substeps, n_mods))
    ev = dto_amd.Evaluator(to_engine(po))
    try:
        r, c = ev.jacobian_structure()
        assert np.array_equal(r, ev_r.jacobian_structure1()[0]) and np.array_equal(c, ev_r.jacobian_structure1()[1])
        r, c = ev.hessian_lagrangian_structure()
        assert np.array_equal(r, ev_r.hessian_structure1()[0]) and np.array_equal(c, ev_r.hessian_structure1()[1])
        g, j, h = _all(ev, po.Z0, mu)
        errs = (rel_err(g, g_r), rel_err(j, j_r), rel_err(h, h_r))
        print("tdb mfma vs reference", n, m, order, substeps, n_mods, errs)
        assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-8, errs
    finally:
        ev.close()


def test_outputs_are_fully_written_and_stay_inside_the_owned_slab():
    """72 states with a DerivativeIntegrator (other rows and components between the integrator's blocks), the middle shard of
    three: device buffers pre-filled with NaN and with guard zones on both sides hold no NaN inside and only NaN outside."""
    import torch
    import dto_amd
    po = _problem(72, 2, 1, 2, 2, N=5, with_derivative=True)
    ev = dto_amd.Evaluator(to_engine(po), k_lo=3, k_hi=4)
    try:
        dev = torch.device("cuda", 0)
        mu = np.random.default_rng(1).standard_normal(ev.n_constraints)
        dZ, dmu = torch.from_numpy(po.Z0).to(dev), torch.from_numpy(mu).to(dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        s, pad = ev.shard, 64
        bufs = [torch.full((ln + 2 * pad,), float("nan"), dtype=torch.float64, device=dev) for ln in (s.cons_len, s.jac_len, s.hess_len)]
        ev.eval_constraint_dev(dZ.data_ptr(), bufs[0].data_ptr() + 8 * pad, st)
        ev.eval_jacobian_dev(dZ.data_ptr(), bufs[1].data_ptr() + 8 * pad, st)
        ev.eval_hessian_dev(dZ.data_ptr(), 0.6, dmu.data_ptr(), bufs[2].data_ptr() + 8 * pad, st)
        torch.cuda.synchronize()
        for b in bufs:
            assert bool(torch.isfinite(b[pad:-pad]).all())
            assert bool(torch.isnan(b[:pad]).all()) and bool(torch.isnan(b[-pad:]).all())
        g, j, h = _all(ev, po.Z0, mu)
        assert np.array_equal(bufs[0][pad:-pad].cpu().numpy(), g) and np.array_equal(bufs[1][pad:-pad].cpu().numpy(), j)
        assert np.array_equal(bufs[2][pad:-pad].cpu().numpy(), h)
    finally:
        ev.close()


def test_more_than_256_states_are_refused_at_create():
    import dto_amd
    po = _problem(272, 1, 0, 2, 0)
    with pytest.raises(Exception, match="256 states"):
        dto_amd.Evaluator(to_engine(po)).close()


def test_sharded_slabs_tile_the_unsharded_vectors_bit_for_bit():
    """An interval's bits depend on the interval alone (not on the grid, the shard or the scratch slot): the slabs of worlds 2 and
    3 tile the unsharded engine's vectors exactly; g through shard_rows()."""
    import dto_amd
    po = _problem(72, 2, 1, 2, 2, N=5)
    p = to_engine(po)
    full = dto_amd.Evaluator(p)
    mu = np.random.default_rng(2).standard_normal(full.n_constraints)
    g, j, h = _all(full, po.Z0, mu)
    full.close()
    for world in (2, 3):
        gj, gh, gg = np.full_like(j, np.nan), np.full_like(h, np.nan), np.full_like(g, np.nan)
        for lo, hi in dto_amd.distributed.shard_ranges(5, world):
            e = dto_amd.Evaluator(p, k_lo=lo, k_hi=hi)
            s = e.shard
            a, b, c = _all(e, po.Z0, mu)
            gj[s.jac_lo:s.jac_lo + s.jac_len] = b
            gh[s.hess_lo:s.hess_lo + s.hess_len] = c
            st, ln = e.shard_rows()
            pos = 0
            for x, y in zip(st, ln):
                gg[x - 1:x - 1 + y] = a[pos:pos + y]
                pos += y
            e.close()
        assert np.array_equal(gj, j) and np.array_equal(gh, h) and np.array_equal(gg, g)


def test_repeated_calls_and_call_history_leave_the_bits_unchanged():
    import dto_amd
    po = _problem(72, 2, 1, 2, 2)
    p = to_engine(po)
    a, b = dto_amd.Evaluator(p), dto_amd.Evaluator(p)
    try:
        mu = np.random.default_rng(3).standard_normal(a.n_constraints)
        g1, j1, h1 = _all(a, po.Z0, mu)      # Hessian after a defect and a Jacobian call
        g2, j2, h2 = _all(a, po.Z0, mu)
        assert np.array_equal(g1, g2) and np.array_equal(j1, j2) and np.array_equal(h1, h2)
        h3 = np.empty(b.shard.hess_len); b.eval_hessian_lagrangian(h3, po.Z0, 0.6, mu)   # fresh handle, Hessian first
        assert np.array_equal(h1, h3)
    finally:
        a.close(); b.close()


def test_time_independent_family_reproduces_the_bilinear_integrator_at_72_states():
    """The construction of test_gpu_time_dependent.py's 3-state test at 72 states, N = 3: no modulation, controls held, so the flow
    is exp(dt G(u)) and the rows agree with a BilinearIntegrator on the same generators to the scheme's error, atol 1e-10 (defect)
    and 1e-9 (Jacobian) as there.  Sub-steps: RK4's global error on a linear flow is about ||M||^5 / (120 S^4) times the flow's
    growth; here ||M|| = dt ||G(u)|| is about 0.2 * 0.7 * 2 sqrt(72) * 1.2 < 3, which at the 3-state test's S = 200 gives 1e-9 --
    above the bar -- and at S = 800 gives 5e-12.  So S is 800 here, the tolerances are the 3-state test's."""
    import dto_amd
    rng = np.random.default_rng(8)
    N, n, m = 3, 72, 1
    traj = dto_amd.NamedTrajectory({"x": rng.standard_normal((n, N)), "u": 0.3 * rng.standard_normal((m, N)),
                                    "t": np.linspace(0, 1, N)[None, :], "dt": np.full((1, N), 0.2)}, timestep="dt")
    G = 0.7 * rng.standard_normal((m + 1, n, n))
    tdb = dto_amd.TimeDependentBilinearIntegrator(dto_amd.ModulatedGenerators(G), "x", "u", "t", traj, spline_order=0, substeps=800)
    bil = dto_amd.BilinearIntegrator(G, "x", "u", traj)
    ev = dto_amd.Evaluator(dto_amd.DirectTrajOptProblem(traj, dto_amd.NullObjective(), [tdb, bil]))
    try:
        Z = traj.vec()
        g = np.empty(ev.n_constraints); ev.eval_constraint(g, Z)
        d = n * (N - 1)
        print("tdb mfma vs exponential: defect", np.abs(g[:d] - g[d:]).max())
        assert np.allclose(g[:d], g[d:], atol=1e-10)
        J = np.empty(ev.n_jacobian_entries); ev.eval_constraint_jacobian(J, Z)
        r, c = ev.jacobian_structure()
        M = np.zeros((ev.n_constraints, ev.n_variables)); M[r - 1, c - 1] = J
        print("tdb mfma vs exponential: Jacobian", np.abs(M[:d] - M[d:]).max())
        assert np.allclose(M[:d], M[d:], atol=1e-9)
    finally:
        ev.close()


def test_products_agree_with_the_dense_products_of_the_values():
    """J w, J' w and the Hessian-vector product go through the slab the value calls fill: wiring only."""
    import dto_amd
    po = _problem(72, 2, 1, 4, 2)
    ev = dto_amd.Evaluator(to_engine(po))
    try:
        rng = np.random.default_rng(5)
        Z = po.Z0
        mu = rng.standard_normal(ev.n_constraints)
        g, j, h = _all(ev, Z, mu)
        r, c = ev.jacobian_structure()
        w, wt, v = rng.standard_normal(ev.n_variables), rng.standard_normal(ev.n_constraints), rng.standard_normal(ev.n_variables)
        y = np.empty(ev.n_constraints); ev.eval_constraint_jacobian_product(y, Z, w)
        ref = np.zeros(ev.n_constraints); np.add.at(ref, r - 1, j * w[c - 1])
        assert rel_err(y, ref) <= 1e-10
        yt = np.empty(ev.n_variables); ev.eval_constraint_jacobian_transpose_product(yt, Z, wt)
        ref = np.zeros(ev.n_variables); np.add.at(ref, c - 1, j * wt[r - 1])
        assert rel_err(yt, ref) <= 1e-10
        hr, hc = ev.hessian_lagrangian_structure()
        yh = np.empty(ev.n_variables); ev.eval_hessian_lagrangian_product(yh, Z, v, 0.6, mu)
        ref = np.zeros(ev.n_variables)
        np.add.at(ref, hr - 1, h * v[hc - 1])
        off = hr != hc
        np.add.at(ref, hc[off] - 1, h[off] * v[hr[off] - 1])
        assert rel_err(yh, ref) <= 1e-8
    finally:
        ev.close()
