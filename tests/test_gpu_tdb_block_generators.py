"""GPU: the TimeDependentBilinearIntegrator with replicated-block generators (DTO_FLAG_BLOCK_GENERATORS, csrc/dto_tdb_kron.hip:
the discrete map of k_tdb / k_tdb_mfma on b x b blocks).

Reference: tests/tdb_large_cases.reference on problems of tests/tdb_block_cases.py -- dense NumPy, pinned to the oracle by
tests/test_tdb_large_reference.py, unaware of the structure.  Bars are those of the other time-dependent tests: 1e-10 max(1, |ref|)
for values and Jacobian, 1e-8 for the Hessian; structure indices bit-exact.  N = 3 (two intervals) unless sharded."""
import numpy as np
import pytest

import dto_oracle as O
import tdb_large_cases as L
from helpers import TOL, TOL_H, rel_err, run_all, to_engine
from tdb_block_cases import kron_tdb_problem, problem_from_family

pytestmark = pytest.mark.gpu

CASES = [(10, 5, 2, 1, 4, 2),    # padded block, n = 50 in k_tdb's range
         (12, 6, 2, 1, 4, 2),    # 72 states
         (16, 8, 2, 1, 3, 0),    # exact tile, no modulation
         (18, 9, 1, 0, 2, 2),    # ragged, two row tiles
         (34, 2, 1, 0, 2, 2),    # three row tiles, r < 16
         (64, 2, 2, 1, 2, 2),    # the block cap
         (64, 8, 1, 0, 2, 1)]    # n = 512


def _all(ev, Z, mu, sigma=0.6):
    g = np.empty(ev.shard.cons_len); ev.eval_constraint(g, Z)
    j = np.empty(ev.shard.jac_len); ev.eval_constraint_jacobian(j, Z)
    h = np.empty(ev.shard.hess_len); ev.eval_hessian_lagrangian(h, Z, sigma, mu)
    return g, j, h


@pytest.mark.parametrize("b,r,m,order,substeps,n_mods", CASES)
def test_structured_path_matches_the_reference(b, r, m, order, substeps, n_mods):
    import dto_amd
    po = kron_tdb_problem(b, r, m, order, substeps, n_mods)
    ev_r, mu, g_r, j_r, h_r = L.reference(po, ("kron", b, r, m, order, substeps, n_mods))
    ev = dto_amd.Evaluator(to_engine(po), block_generators=True)
    try:
        assert ev.integrator_blocks(0) == (b, r, 1)
        rr, cc = ev.jacobian_structure()
        assert np.array_equal(rr, ev_r.jacobian_structure1()[0]) and np.array_equal(cc, ev_r.jacobian_structure1()[1])
        rr, cc = ev.hessian_lagrangian_structure()
        assert np.array_equal(rr, ev_r.hessian_structure1()[0]) and np.array_equal(cc, ev_r.hessian_structure1()[1])
        g, j, h = _all(ev, po.Z0, mu)
        errs = (rel_err(g, g_r), rel_err(j, j_r), rel_err(h, h_r))
        print("tdb kron vs reference", b, r, m, order, substeps, n_mods, errs)
        assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-8, errs
    finally:
        ev.close()


def test_profile_tells_which_path_ran():
    import dto_amd
    po = kron_tdb_problem(16, 8, 2, 1, 3, 0)
    p = to_engine(po)
    mu = np.random.default_rng(1).standard_normal(2 * 128)
    for flag, ran, idle in ((True, "tdb_kron", "tdb_mfma"), (False, "tdb_mfma", "tdb_kron")):
        ev = dto_amd.Evaluator(p, block_generators=flag)
        try:
            ev.profile_enable(True)
            for call in range(3):
                ev.profile_reset()
                if call == 0:
                    g = np.empty(ev.n_constraints); ev.eval_constraint(g, po.Z0)
                elif call == 1:
                    j = np.empty(ev.n_jacobian_entries); ev.eval_constraint_jacobian(j, po.Z0)
                else:
                    h = np.empty(ev.n_hessian_entries); ev.eval_hessian_lagrangian(h, po.Z0, 0.6, mu)
                ms, launches, flops = ev.profile_get(ran)
                assert launches == 1 and flops > 0.0, (flag, call, launches)
                assert ev.profile_get(idle)[1] == 0
                assert ev.profile_get("all")[1] >= 1
        finally:
            ev.close()


@pytest.mark.parametrize("b,r,m,order,substeps,n_mods", [(12, 6, 2, 1, 4, 2), (16, 8, 2, 1, 3, 0)])
def test_flagged_and_unflagged_handles_agree(b, r, m, order, substeps, n_mods):
    """To the bars, not bit for bit: the summation orders differ."""
    import dto_amd
    po = kron_tdb_problem(b, r, m, order, substeps, n_mods)
    p = to_engine(po)
    a, d = dto_amd.Evaluator(p, block_generators=True), dto_amd.Evaluator(p)
    try:
        assert a.integrator_blocks(0) == (b, r, 1) and d.integrator_blocks(0) == (b * r, 1, 0)
        mu = np.random.default_rng(3).standard_normal(a.n_constraints)
        errs = [rel_err(x, y) for x, y in zip(_all(a, po.Z0, mu), _all(d, po.Z0, mu))]
        print("tdb kron vs dense path", b, r, errs)
        assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-8, errs
    finally:
        a.close(); d.close()


def test_flag_without_structure_returns_the_unflagged_bits():
    import dto_amd
    po = O.make_tdb_problem(N=3, n=72, m=2, order=1, seed=112, substeps=2, n_mods=2)
    p = to_engine(po)
    a, d = dto_amd.Evaluator(p, block_generators=True), dto_amd.Evaluator(p)
    try:
        assert a.integrator_blocks(0) == (72, 1, 0)
        mu = np.random.default_rng(4).standard_normal(a.n_constraints)
        for x, y in zip(_all(a, po.Z0, mu), _all(d, po.Z0, mu)):
            assert np.array_equal(x, y)
    finally:
        a.close(); d.close()


def test_outputs_are_fully_written_inside_the_slab_twice_in_a_row():
    """12 x 6 with a DerivativeIntegrator between the blocks, N = 5, the middle shard of three; device buffers pre-filled with NaN
    and guarded on both sides; two rounds at two points: the constant zeros of the staged blocks survive a call and every owned
    entry is assigned again (the second round equals a fresh handle's values at the second point)."""
    import torch
    import dto_amd
    po = kron_tdb_problem(12, 6, 2, 1, 2, 2, N=5, with_derivative=True)
    p = to_engine(po)
    ev = dto_amd.Evaluator(p, k_lo=3, k_hi=4, block_generators=True)
    try:
        assert ev.integrator_blocks(0) == (12, 6, 1)
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(1)
        mu = rng.standard_normal(ev.n_constraints)
        Zs = [po.Z0, po.Z0 + 0.05 * rng.standard_normal(po.Z0.size)]
        dmu = torch.from_numpy(mu).to(dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        s, pad = ev.shard, 64
        for Z in Zs:
            dZ = torch.from_numpy(Z).to(dev)
            bufs = [torch.full((ln + 2 * pad,), float("nan"), dtype=torch.float64, device=dev) for ln in (s.cons_len, s.jac_len, s.hess_len)]
            ev.eval_constraint_dev(dZ.data_ptr(), bufs[0].data_ptr() + 8 * pad, st)
            ev.eval_jacobian_dev(dZ.data_ptr(), bufs[1].data_ptr() + 8 * pad, st)
            ev.eval_hessian_dev(dZ.data_ptr(), 0.6, dmu.data_ptr(), bufs[2].data_ptr() + 8 * pad, st)
            torch.cuda.synchronize()
            for b in bufs:
                assert bool(torch.isfinite(b[pad:-pad]).all())
                assert bool(torch.isnan(b[:pad]).all()) and bool(torch.isnan(b[-pad:]).all())
            fresh = dto_amd.Evaluator(p, k_lo=3, k_hi=4, block_generators=True)
            try:
                for mine, ref in zip(bufs, _all(fresh, Z, mu)):
                    assert np.array_equal(mine[pad:-pad].cpu().numpy(), ref)
            finally:
                fresh.close()
        # and the values are the dense path's to the bars (the zeros outside the diagonal blocks exactly)
        d = dto_amd.Evaluator(p, k_lo=3, k_hi=4)
        try:
            ref = _all(d, Zs[1], mu)
            mine = [b[pad:-pad].cpu().numpy() for b in bufs]
            assert rel_err(mine[0], ref[0]) <= 1e-10 and rel_err(mine[1], ref[1]) <= 1e-10 and rel_err(mine[2], ref[2]) <= 1e-8
            assert np.all(mine[1][ref[1] == 0.0] == 0.0)
        finally:
            d.close()
    finally:
        ev.close()


def test_sharded_slabs_tile_the_unsharded_vectors_bit_for_bit():
    import dto_amd
    po = kron_tdb_problem(12, 6, 2, 1, 2, 2, N=5)
    p = to_engine(po)
    full = dto_amd.Evaluator(p, block_generators=True)
    mu = np.random.default_rng(2).standard_normal(full.n_constraints)
    g, j, h = _all(full, po.Z0, mu)
    full.close()
    for world in (2, 3):
        gj, gh, gg = np.full_like(j, np.nan), np.full_like(h, np.nan), np.full_like(g, np.nan)
        for lo, hi in dto_amd.distributed.shard_ranges(5, world):
            e = dto_amd.Evaluator(p, k_lo=lo, k_hi=hi, block_generators=True)
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
    po = kron_tdb_problem(12, 6, 2, 1, 2, 2)
    p = to_engine(po)
    a, b = dto_amd.Evaluator(p, block_generators=True), dto_amd.Evaluator(p, block_generators=True)
    try:
        mu = np.random.default_rng(3).standard_normal(a.n_constraints)
        g1, j1, h1 = _all(a, po.Z0, mu)
        g2, j2, h2 = _all(a, po.Z0, mu)
        assert np.array_equal(g1, g2) and np.array_equal(j1, j2) and np.array_equal(h1, h2)
        h3 = np.empty(b.shard.hess_len); b.eval_hessian_lagrangian(h3, po.Z0, 0.6, mu)   # fresh handle, Hessian first
        assert np.array_equal(h1, h3)
    finally:
        a.close(); b.close()


def _to_oracle(prob):
    """The oracle's statement of synthetic.unitary_tdb_problem."""
    import dto_amd
    traj = prob.trajectory
    z, dt_idx = traj.dim, traj.components[traj.timestep][0]
    integ = []
    for it in prob.integrators:
        if isinstance(it, dto_amd.TimeDependentBilinearIntegrator):
            fam = it.family
            integ.append(O.TimeDependentBilinearIntegrator(it.x_off, traj.dims[it.x_name], it.u_off, it.u_dim, it.t_off, fam.G, fam.mods,
                                                           it.spline_order, it.substeps).bind(z, dt_idx))
        else:
            integ.append(O.DerivativeIntegrator(it.x_off, it.x_dim, it.xdot_off))
    terms, weights = [], []
    for o, w in zip(prob.objective.objectives, prob.objective.weights):
        if isinstance(o, dto_amd.QuadraticRegularizer):
            terms.append(O.QuadraticRegularizer(o.comp_off, o.comp_dim, np.asarray(o.R)))
        else:
            terms.append(O.LowRankInfidelityObjective(list(o.comps), list(o.times), list(o.Qs), o.A))
        weights.append(w)
    return O.Problem(N=traj.N, z=z, dt_idx=dt_idx, integrators=integ, objectives=terms, weights=weights,
                     Z0=np.ascontiguousarray(traj.vec(), dtype=np.float64))


def test_unitary_tdb_problem_matches_the_oracle_and_the_dev_forms_agree():
    """All five callbacks of synthetic.unitary_tdb_problem (6 levels: 72 states, blocks 12 x 6) against the oracle's evaluator with
    the integrator's blocks in the fast form of tests/tdb_large_cases.py; the device-pointer forms return the host-pointer bits."""
    import torch
    import dto_amd
    pe = dto_amd.synthetic.unitary_tdb_problem(levels=6, drives=2, N=4)
    po = _to_oracle(pe)
    ev_o = O.OracleEvaluator(L.fast_problem(po))
    ev = dto_amd.Evaluator(pe, block_generators=True)
    try:
        assert ev.integrator_blocks(0) == (12, 6, 1)
        for mine, ref in ((ev.jacobian_structure(), ev_o.jacobian_structure1()), (ev.hessian_lagrangian_structure(), ev_o.hessian_structure1())):
            assert np.array_equal(mine[0], ref[0]) and np.array_equal(mine[1], ref[1])
        Z = po.Z0
        mu = np.random.default_rng(5).standard_normal(ev_o.n_constraints)
        out = run_all(ev, po, Z, mu, sigma=0.7, hessian=True)
        errs = {"f": rel_err(out["f"], ev_o.eval_objective(Z)), "grad": rel_err(out["grad"], ev_o.eval_objective_gradient(Z)),
                "cons": rel_err(out["cons"], ev_o.eval_constraint(Z)), "jac": rel_err(out["jac"], ev_o.eval_constraint_jacobian(Z)),
                "hess": rel_err(out["hess"], ev_o.eval_hessian_lagrangian(Z, 0.7, mu))}
        print("unitary tdb", errs)
        for k, v in errs.items():
            assert v <= (TOL_H if k == "hess" else TOL), (k, v)
        dev = torch.device("cuda", 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        dZ, dmu = torch.from_numpy(Z).to(dev), torch.from_numpy(mu).to(dev)
        f = torch.empty(1, dtype=torch.float64, device=dev)
        grad = torch.empty(ev.n_variables, dtype=torch.float64, device=dev)
        g = torch.empty(ev.n_constraints, dtype=torch.float64, device=dev)
        J = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dev)
        H = torch.empty(ev.n_hessian_entries, dtype=torch.float64, device=dev)
        ev.eval_objective_dev(dZ.data_ptr(), f.data_ptr(), st)
        ev.eval_gradient_dev(dZ.data_ptr(), grad.data_ptr(), st)
        ev.eval_constraint_dev(dZ.data_ptr(), g.data_ptr(), st)
        ev.eval_jacobian_dev(dZ.data_ptr(), J.data_ptr(), st)
        ev.eval_hessian_dev(dZ.data_ptr(), 0.7, dmu.data_ptr(), H.data_ptr(), st)
        torch.cuda.synchronize()
        assert float(f.cpu()[0]) == out["f"]
        for mine, ref in ((grad, out["grad"]), (g, out["cons"]), (J, out["jac"]), (H, out["hess"])):
            assert np.array_equal(mine.cpu().numpy(), ref)
    finally:
        ev.close()
