"""GPU: bilinear integrators whose generators are replicated blocks, G_j = I_r (x) B_j (DTO_FLAG_BLOCK_GENERATORS, csrc/dto_kron.hip).
The expected values are those of the oracle's BilinearIntegrator with G = kron(I_r, B): tolerances 1e-10 max(1, |ref|) for
objective, gradient, constraint and Jacobian, 1e-8 max(1, |ref|) for the Hessian, indices bit-exact."""
import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import TOL, TOL_H, host_getter, rel_err, run_all, sampled_checks, to_engine

pytestmark = pytest.mark.gpu


def kron_problem(b, r, m, N, seed=0, extra_dense=0):
    """x[b r], u[m], du[m], (y[extra_dense],) dt: the scaling generator's shape with G_j = kron(I_r, B_j); `extra_dense` adds a
    second bilinear integrator with dense generators on a component of its own, driven by the same controls."""
    rng = np.random.default_rng(seed)
    n = b * r
    B = rng.standard_normal((m + 1, b, b)) / np.sqrt(b)
    G = np.stack([np.kron(np.eye(r), Bj) for Bj in B])
    z = n + 2 * m + extra_dense + 1
    Zk = rng.standard_normal((N, z))
    Zk[:, n:n + m] *= 0.3
    Zk[:, z - 1] = 0.1 + 0.05 * rng.random(N)
    integ = [O.BilinearIntegrator(0, n, n, m, G), O.DerivativeIntegrator(n, m, n + m)]
    if extra_dense:
        Gd = rng.standard_normal((m + 1, extra_dense, extra_dense)) / np.sqrt(extra_dense)
        integ.append(O.BilinearIntegrator(n + 2 * m, extra_dense, n, m, Gd))
    return O.Problem(N=N, z=z, dt_idx=z - 1, integrators=integ, objectives=[O.QuadraticRegularizer(n, m, np.ones(m))],
                     Z0=Zk.reshape(-1).copy())


def to_oracle(prob):
    """The oracle's statement of a host-mirror problem made of the built-in kinds synthetic.unitary_problem uses."""
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
            terms.append(O.LowRankInfidelityObjective(list(o.comps), list(o.times), list(o.Qs), o.A))
        weights.append(w)
    cons = [O.KnotConstraint(c.kind, list(c.comps), c.c, list(c.times), c.equality) for c in prob.constraints]
    return O.Problem(N=traj.N, z=traj.dim, dt_idx=traj.components[traj.timestep][0], integrators=integ, objectives=terms,
                     weights=weights, constraints=cons, Z0=np.ascontiguousarray(traj.vec(), dtype=np.float64))


def check_all(prob_o, prob_e, blocks, tag, hessian_full=True):
    """f, grad f, g, J, H, J w, J' w, H v of a flagged handle against the oracle."""
    ev_o = O.OracleEvaluator(prob_o)
    ev = dto_amd.Evaluator(prob_e, block_generators=True)
    try:
        assert ev.integrator_blocks(0) == blocks, ev.integrator_blocks(0)
        for mine, ref in ((ev.jacobian_structure(), ev_o.jacobian_structure1()), (ev.hessian_lagrangian_structure(), ev_o.hessian_structure1())):
            assert np.array_equal(mine[0], ref[0]) and np.array_equal(mine[1], ref[1])
        rng = np.random.default_rng(2)
        Z = prob_o.Z0
        mu = rng.standard_normal(ev_o.n_constraints)
        out = run_all(ev, prob_o, Z, mu, sigma=0.7, hessian=True)
        errs = {"f": rel_err(out["f"], ev_o.eval_objective(Z)), "grad": rel_err(out["grad"], ev_o.eval_objective_gradient(Z)),
                "cons": rel_err(out["cons"], ev_o.eval_constraint(Z)), "jac": rel_err(out["jac"], ev_o.eval_constraint_jacobian(Z))}
        w = rng.standard_normal(prob_o.n_vars)
        y = np.full(ev_o.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, Z, w)
        errs["Jw"] = rel_err(y, ev_o.eval_constraint_jacobian_product(Z, w))
        wt = rng.standard_normal(ev_o.n_constraints)
        y = np.full(prob_o.n_vars, np.nan); ev.eval_constraint_jacobian_transpose_product(y, Z, wt)
        errs["JTw"] = rel_err(y, ev_o.eval_constraint_jacobian_transpose_product(Z, wt))
        hv = np.full(prob_o.n_vars, np.nan); ev.eval_hessian_lagrangian_product(hv, Z, w, 0.7, mu)
        if hessian_full:
            Href = ev_o.eval_hessian_lagrangian(Z, 0.7, mu)
            errs["hess"] = rel_err(out["hess"], Href)
            r1, c1 = ev_o.hessian_structure1()
            Hd = np.zeros((prob_o.n_vars, prob_o.n_vars)); Hd[r1 - 1, c1 - 1] = Href
            errs["Hv"] = rel_err(hv, (Hd + np.triu(Hd, 1).T) @ w)
        else:  # the product against the engine's own Hessian (the oracle's is checked on sampled blocks by the caller)
            r1, c1 = ev.hessian_lagrangian_structure()
            ref = np.zeros(prob_o.n_vars)
            np.add.at(ref, r1 - 1, out["hess"] * w[c1 - 1])
            off = r1 != c1
            np.add.at(ref, c1[off] - 1, out["hess"][off] * w[r1[off] - 1])
            errs["Hv"] = rel_err(hv, ref)
        print(tag, errs, ev.last_stats())
        for k, v in errs.items():
            assert v <= (TOL_H if k in ("hess", "Hv") else TOL), (tag, k, v)
        return out, mu
    finally:
        ev.close()


@pytest.mark.parametrize("b,r,m,N", [(16, 4, 2, 6), (12, 6, 3, 5), (20, 5, 1, 4), (64, 3, 4, 4)])
def test_callbacks_match_the_oracle(b, r, m, N):
    p = kron_problem(b, r, m, N, seed=b + r)
    check_all(p, to_engine(p), (b, r, 1), f"kron {b}x{r} m={m}")


def test_callbacks_match_the_oracle_512_states():
    """b = 32, r = 16, m = 4, three knots: every callback in full (the oracle's side takes about ten seconds), and the Hessian once
    more on the blocks of the sampled two-knot helpers."""
    b, r, m, N = 32, 16, 4, 3
    p = kron_problem(b, r, m, N, seed=48)
    pe = to_engine(p)
    out, mu = check_all(p, pe, (b, r, 1), "kron 32x16 m=4")
    ev = dto_amd.Evaluator(pe, block_generators=True)
    try:
        sampled_checks(pe, ev, b * r, m, [0, 2], hess_get=host_getter(out["hess"]), mu=mu, sigma=0.7)
    finally:
        ev.close()


def unitary(N=12):
    # knot 2: a step of 3.0 (||A|| ~ 6: the series runs past its hump, and the dense path squares); knot 3: 1e-4 (a few terms)
    return dto_amd.synthetic.unitary_problem(levels=8, drives=2, N=N, seed=5, dt_large=3.0, dt_small=1e-4)


def test_unitary_problem_matches_the_oracle():
    pe = unitary()
    check_all(to_oracle(pe), pe, (16, 8, 1), "unitary 8 levels")


def test_flagged_and_unflagged_handles_agree():
    pe = unitary()
    a, d = dto_amd.Evaluator(pe, block_generators=True), dto_amd.Evaluator(pe)
    try:
        assert a.integrator_blocks(0) == (16, 8, 1) and d.integrator_blocks(0) == (128, 1, 0)
        Z = pe.trajectory.vec()
        mu = np.random.default_rng(3).standard_normal(a.n_constraints)
        oa, od = run_all(a, None, Z, mu, 0.7), run_all(d, None, Z, mu, 0.7)
        errs = {k: rel_err(oa[k], od[k]) for k in oa}
        print(errs)
        assert errs["hess"] <= TOL_H and all(errs[k] <= TOL for k in ("f", "grad", "cons", "jac")), errs
        # the share (r-1)/r of every x-block is the same structural zero on both
        assert np.all(oa["jac"][od["jac"] == 0.0] == 0.0)
    finally:
        a.close(); d.close()


def test_repeated_calls_are_bit_identical():
    import torch
    pe = unitary()
    ev = dto_amd.Evaluator(pe, block_generators=True)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        dZ = torch.from_numpy(pe.trajectory.vec()).to(dev)
        dmu = torch.from_numpy(np.random.default_rng(4).standard_normal(ev.n_constraints)).to(dev)
        runs = []
        for _ in range(3):
            g = torch.full((ev.shard.cons_len,), float("nan"), dtype=torch.float64, device=dev)
            J = torch.full((ev.shard.jac_len,), float("nan"), dtype=torch.float64, device=dev)
            H = torch.full((ev.shard.hess_len,), float("nan"), dtype=torch.float64, device=dev)
            ev.eval_constraint_dev(dZ.data_ptr(), g.data_ptr(), st)
            ev.eval_jacobian_dev(dZ.data_ptr(), J.data_ptr(), st)
            ev.eval_hessian_dev(dZ.data_ptr(), 0.7, dmu.data_ptr(), H.data_ptr(), st)
            torch.cuda.synchronize()
            runs.append((g, J, H))
        for other in runs[1:]:
            for x, y in zip(runs[0], other):
                assert torch.equal(x, y)
    finally:
        ev.close()


def test_shards_are_slices_of_the_whole():
    pe = unitary()
    Z = pe.trajectory.vec()
    whole = dto_amd.Evaluator(pe, block_generators=True)
    try:
        mu = np.random.default_rng(6).standard_normal(whole.n_constraints)
        ow = run_all(whole, None, Z, mu, 0.7)
        for lo, hi in ((1, 5), (6, 12)):
            ev = dto_amd.Evaluator(pe, block_generators=True, k_lo=lo, k_hi=hi)
            try:
                assert ev.integrator_blocks(0) == (16, 8, 1)
                o = run_all(ev, None, Z, mu, 0.7)
                s = ev.shard
                assert np.array_equal(o["jac"], ow["jac"][s.jac_lo:s.jac_lo + s.jac_len])
                assert np.array_equal(o["hess"], ow["hess"][s.hess_lo:s.hess_lo + s.hess_len])
                assert np.array_equal(o["grad"], ow["grad"][s.grad_lo:s.grad_lo + s.grad_len])
                starts, lens = ev.shard_rows()
                ref = np.concatenate([ow["cons"][a - 1:a - 1 + n] for a, n in zip(starts, lens)])
                assert np.array_equal(o["cons"], ref)
            finally:
                ev.close()
    finally:
        whole.close()


def test_bound_output_keeps_constants_and_tracks_the_point():
    """Poisoned variable entries, two points: every entry is right after each call; the zero share of the x-blocks is a constant of
    the plan -- poisoning everything that demonstrably varies does not reach it, and it is not among the cleared runs."""
    import torch
    from dto_amd import capi
    pe = unitary()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    ev, ref = dto_amd.Evaluator(pe, block_generators=True), dto_amd.Evaluator(pe, block_generators=True)
    try:
        rng = np.random.default_rng(0)
        Z0 = pe.trajectory.vec()
        Zs = [Z0 + 0.05 * k * rng.standard_normal(Z0.size) for k in range(3)]
        dZ = [torch.from_numpy(Z).to(dev) for Z in Zs]
        dmu = [torch.from_numpy(rng.standard_normal(ev.n_constraints)).to(dev) for _ in range(3)]

        def call(e, k, which, o):
            if which == "jac":
                e.eval_jacobian_dev(dZ[k].data_ptr(), o.data_ptr(), st)
            else:
                e.eval_hessian_dev(dZ[k].data_ptr(), 0.7, dmu[k].data_ptr(), o.data_ptr(), st)
            torch.cuda.synchronize()

        for which, vec in (("jac", capi.VECTOR_JACOBIAN), ("hess", capi.VECTOR_HESSIAN)):
            n = ref.shard.jac_len if which == "jac" else ref.shard.hess_len
            want = []
            for k in range(3):
                o = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
                call(ref, k, which, o)
                want.append(o)
            varies = (want[0] != want[1]) | (want[0] != want[2])
            assert 0 < int(varies.sum()) < n
            buf = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
            ev.bind_output_dev(vec, buf.data_ptr())
            for k in (0, 1, 2, 0):
                call(ev, k, which, buf)
                assert torch.equal(buf, want[k]), (which, k, int((buf != want[k]).sum()))
                buf[varies] = float("nan")
            if which == "jac":
                # a constant zero of an x-block marked after priming survives the next call: the call did not rewrite it
                pos = 16  # first column of the first knot, row 16 of interval 1: outside the column's own 16 x 16 block
                assert want[0][pos] == 0.0 and want[1][pos] == 0.0
                call(ev, 0, which, buf)
                buf[pos] = 7.0
                call(ev, 1, which, buf)
                assert buf[pos] == 7.0
                buf[pos] = 0.0
                assert torch.equal(buf, want[1])
            ev.bind_output_dev(vec, 0)
    finally:
        ev.close(); ref.close()


def test_structured_and_dense_integrators_side_by_side():
    p = kron_problem(16, 4, 2, 5, seed=9, extra_dense=40)
    pe = to_engine(p)
    ev = dto_amd.Evaluator(pe, block_generators=True)
    try:
        assert ev.integrator_blocks(0) == (16, 4, 1) and ev.integrator_blocks(2) == (40, 1, 0)
    finally:
        ev.close()
    check_all(p, pe, (16, 4, 1), "kron 16x4 + dense 40")
