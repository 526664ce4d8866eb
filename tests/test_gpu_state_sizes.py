"""GPU: 257..1023 states against the oracle -- the sizes between the 256-state tests and the 1024-state workload -- and 65 states
on 3489 / 3509 intervals, the one place where a launch's LENGTH chooses between the two batched-GEMM kernels.

Above 256 states the engine runs code of its own: padding to npad = pad64(n) with the chain's GEMMs on 64 x 64 tiles where
npad % 128 != 0 (320, 448, 576, 704, 832, 960) and the sweeps 64 columns wide; the persistent ring core on 128 x 128 tiles
where npad % 128 == 0 (384: 9 tiles per matrix, 512: 16, 768: 36), its grid wrapping round at 512 tiles; step-per-launch
sweeps (the fused, cluster and generator-stationary forms refuse), k_pair_combine / k_hess_pair<m> for the (u, u) block;
from 512 on, no overlap of sweep and chain.  The oracle's (u, u) terms above 256 states come from the complex step on
scipy's expm_frechet (oracle/dto_oracle.py _second_frechet_action_cs, pinned in test_oracle_pinning.py).

Every case also asserts, through the profile counters and last_stats, that it ran the path it is there for.
Tolerances as everywhere: 1e-10 max(1,|ref|) values / Jacobian, 1e-8 Hessian, sparsity bit-exact."""
import numpy as np
import pytest

import dto_oracle as O
from helpers import assert_sweep_form, check_callbacks, host_getter, sampled_checks, sweep_forms, to_engine

pytestmark = pytest.mark.gpu


def _launches(ev, name):
    return ev.profile_get(name)[1]


def _path_counts(prob_o, Z, hessian=True):
    """Profile launch counts of one Jacobian and (separately) one Hessian call of a fresh handle, and last_stats after each."""
    import dto_amd
    ev = dto_amd.Evaluator(to_engine(prob_o), eval_hessian=hessian)
    try:
        ev.profile_enable(True)
        ev.profile_reset()
        j = np.empty(ev.n_jacobian_entries); ev.eval_constraint_jacobian(j, Z)
        out = {"jac": {k: _launches(ev, k) for k in ("basis_multi", "bgemm_square", "bgemm_plain", "chain64", "expmv")},
               "jac_stats": ev.last_stats(), "forms": {"J": sweep_forms(ev)}}
        ev.profile_reset()
        g = np.empty(ev.n_constraints); ev.eval_constraint(g, Z)
        out["forms"]["g"] = sweep_forms(ev)
        if hessian:
            ev.profile_reset()
            mu = np.random.default_rng(0).standard_normal(ev.n_constraints)
            h = np.empty(ev.n_hessian_entries); ev.eval_hessian_lagrangian(h, Z, 0.7, mu)
            out["hess"] = {k: _launches(ev, k) for k in ("expmv", "expmv_adjoint")}
            out["forms"]["H"] = sweep_forms(ev)
        return out
    finally:
        ev.close()


def _assert_large_state_chain(counts):
    """The chain of a > 256-state integrator: generator-subspace powers once per chunk, batched-GEMM squarings (dt = 0.1 puts
    alpha past the radius of either polynomial form at these sizes), no one-launch 64-state chain."""
    c = counts["jac"]
    assert c["basis_multi"] >= 1 and c["chain64"] == 0, counts
    for what, f in counts["forms"].items():   # every sweep one launch per Taylor step: the one-launch forms refuse these sizes
        assert_sweep_form(f, "step", what=what)
    assert c["bgemm_square"] >= 1 and counts["jac_stats"][0] >= 1, counts


@pytest.mark.parametrize("n,m", [(300, 1), (384, 3), (448, 2), (512, 4), (700, 5), (960, 2)])
def test_every_callback_between_256_and_1024_states(n, m):
    """Three knots, ||u|| - 1 <= 0 at the middle one: f, gradient, constraints, Jacobian, J w, J' w and the whole Hessian
    ((u, u) included) against the oracle.  300: npad 320, 20 padded rows; 384: ring core, 3 x 3 tiles; 448: 64-tile GEMMs;
    512: ring core 4 x 4, no sweep / chain overlap, exact_d2(higher) planning; 700: npad 704, 11 x 11 tiles of 64; 960: the
    widest 64-tile pitch.  m = 1..5: five instances of k_hess_pair<m>."""
    p = O.make_scaled_problem(3, n, m, seed=n + m, with_constraint=True)
    check_callbacks(p, seed=n, tag=f"n={n} m={m}", products=True)
    counts = _path_counts(p, p.Z0)
    print(counts)
    _assert_large_state_chain(counts)
    assert counts["hess"]["expmv"] >= 1 and counts["hess"]["expmv_adjoint"] >= 1, counts


@pytest.mark.parametrize("n,m,N,ks", [
    # 384 states, 199 intervals: 9 ring tiles per matrix, 1800 tiles (batches padded to 8) in rounds of 512 -- interval 60 is cut
    # between rounds 0 and 1, 100 lies inside round 1, 115 is cut between rounds 1 and 2, 170 between rounds 2 and 3, and the last
    # round holds the remainder
    (384, 2, 200, (0, 1, 60, 100, 115, 170, 198, 199)),
    # npad 320: every chain GEMM on 64 x 64 tiles (25 per matrix), the sweeps 64 columns wide
    (320, 2, 200, (0, 1, 64, 137, 198, 199)),
    # npad 512: 16 ring tiles per matrix, 63 intervals -> exactly two rounds; no overlap of sweep and chain
    (512, 4, 64, (0, 1, 31, 32, 62, 63)),
])
def test_longer_horizons_sampled(n, m, N, ks):
    """Long enough for the chain's launches to cover many intervals: Jacobian column blocks, defects and Hessian diagonal blocks
    of sampled knots (first and last among them) against two-knot oracle problems."""
    import dto_amd
    prob = dto_amd.host.synthetic.make_scaled_problem(N, n, m, seed=n)
    ev = dto_amd.Evaluator(prob)
    try:
        Z = prob.trajectory.vec()
        mu = np.random.default_rng(n).standard_normal(ev.n_constraints)
        ev.profile_enable(True)
        ev.profile_reset()
        jac = np.full(ev.n_jacobian_entries, np.nan); ev.eval_constraint_jacobian(jac, Z)
        squares, chunks = _launches(ev, "bgemm_square"), _launches(ev, "basis_multi")
        squarings = ev.last_stats()[0]
        assert_sweep_form(sweep_forms(ev), "step", what="Jacobian")
        ev.profile_enable(False)
        assert chunks == 1 and squares >= 1 and squarings >= 1, (chunks, squares, squarings)
        cons = np.full(ev.n_constraints, np.nan); ev.eval_constraint(cons, Z)
        hes = np.full(ev.n_hessian_entries, np.nan); ev.eval_hessian_lagrangian(hes, Z, 0.7, mu)
        assert np.isfinite(jac).all() and np.isfinite(cons).all() and np.isfinite(hes).all()
        sampled_checks(prob, ev, n, m, ks, host_getter(jac), host_getter(hes), cons, mu, 0.7)
    finally:
        ev.close()


def test_large_steps_at_384_states_take_substeps_and_leave_the_pairing_path():
    """Big time steps (||A_k||_1 up to ~150): many squarings in the chain, the sweeps need q > 1 rounds, which takes the Hessian
    off the pairing path onto second-order columns (its forward sweep then carries every column type in one launch sequence)."""
    p = O.make_scaled_problem(4, 384, 2, seed=29, with_constraint=True)
    Z = p.Z0.copy()
    Z[p.dt_idx::p.z] = [0.5, 0.2, 0.35, 0.1]
    check_callbacks(p, Z=Z, seed=3, tag="n=384 large steps", products=True)
    big = _path_counts(p, Z)
    small = _path_counts(p, p.Z0)
    print("large steps", big, "dt = 0.1", small)
    _assert_large_state_chain(big)
    assert big["jac_stats"][0] > small["jac_stats"][0], (big, small)
    # pairing path: the forward p column and the pairing products are two timed regions of kind expmv; second-order columns: one
    assert small["hess"]["expmv"] == 2 and big["hess"]["expmv"] == 1, (big, small)


@pytest.mark.parametrize("N,kernel", [(3490, "64-tile"), (3510, "ring")])
def test_one_tile_per_matrix_on_both_sides_of_the_3500_interval_crossover(N, kernel):
    """65 states (npad 128: ONE 128-tile per matrix), 1 drive, default options.  With a single tile per matrix the batched GEMMs take
    the 64-tile kernel below 3500 intervals in the launch and the ring kernel from 3500 on (csrc/dto_bgemm_dispatch.h; the rule
    itself is checked by test_bgemm_dispatch_header.py): 3489 intervals in one launch run the first, 3509 the second -- the ring
    kernel with tiles_r = 1, its persistent grid of 512 wrapping round 3512 slots.
    The launch holds all the intervals only when the chain runs as ONE chunk, which the device-pointer Jacobian does (asserted through
    the count of generator-subspace launches); the host-pointer eval_constraint_jacobian cuts the chain into four chunks for its early
    hand-over of finished blocks (880 intervals per launch: the 64-tile kernel at either length).  Both are evaluated and both compared:
    Jacobian column blocks (and the chain-vs-sweep cross check) of six intervals against two-knot oracle problems -- the first, the
    last, both sides of the first wrap of the persistent grid (slots 511 | 512), and two inside later rounds."""
    import torch
    import dto_amd
    n, m, K = 65, 1, N - 1
    ks = (0, 511, 512, 1777, 3072, K - 1)
    prob = dto_amd.host.synthetic.make_scaled_problem(N, n, m, seed=N)
    ev = dto_amd.Evaluator(prob, eval_hessian=False)
    try:
        Z = prob.trajectory.vec()
        cons = np.full(ev.n_constraints, np.nan); ev.eval_constraint(cons, Z)
        assert np.isfinite(cons).all()
        ev.profile_enable(True)
        # host pointers, default options (what a solver calls)
        ev.profile_reset()
        jac = np.full(ev.n_jacobian_entries, np.nan); ev.eval_constraint_jacobian(jac, Z)
        host_chunks = _launches(ev, "basis_multi")
        assert np.isfinite(jac).all() and _launches(ev, "chain64") == 0
        sampled_checks(prob, ev, n, m, ks, host_getter(jac), None, cons)
        del jac
        # device pointers: one chunk, every batched GEMM of the chain a launch of K intervals
        dev = torch.device("cuda", 0)
        dZ = torch.from_numpy(Z).to(dev)
        dj = torch.full((ev.n_jacobian_entries,), float("nan"), dtype=torch.float64, device=dev)
        ev.profile_reset()
        ev.eval_jacobian_dev(dZ.data_ptr(), dj.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        dev_chunks = _launches(ev, "basis_multi")
        ev.profile_enable(False)
        print(kernel, "chunks: host form", host_chunks, "device form", dev_chunks, ev.last_stats())
        assert dev_chunks == 1 and _launches(ev, "chain64") == 0, (host_chunks, dev_chunks)
        assert bool(torch.isfinite(dj).all())
        sampled_checks(prob, ev, n, m, ks, lambda lo, hi: dj[lo:hi].cpu().numpy(), None, cons)
        del dj
    finally:
        ev.close()
