"""GPU: bilinear integrators with equal generators and controls share one propagator chain (DTO_FLAG_SHARED_GENERATORS,
csrc/dto_share.hip).  Every case is synthetic.multi_ket_problem with a knot constraint on u, whose entries interleave with the
integrators' in the u columns.  Tolerances against the oracle: 1e-10 max(1, |ref|) for objective, gradient, constraint, Jacobian,
J w and J' w, 1e-8 max(1, |ref|) for the Hessian; against the unflagged handle: bit for bit where stated."""
import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import TOL, TOL_H, rel_err, run_all
from multi_ket_cases import e_block_index, multi_ket, to_oracle

pytestmark = pytest.mark.gpu


def check_against_oracle(pe, want_share, tag):
    po = to_oracle(pe)
    ev_o = O.OracleEvaluator(po)
    ev = dto_amd.Evaluator(pe, shared_generators=True)
    try:
        assert [ev.integrator_share(i) for i in range(len(pe.integrators))] == want_share
        for mine, ref in ((ev.jacobian_structure(), ev_o.jacobian_structure1()), (ev.hessian_lagrangian_structure(), ev_o.hessian_structure1())):
            assert np.array_equal(mine[0], ref[0]) and np.array_equal(mine[1], ref[1])
        rng = np.random.default_rng(2)
        Z = po.Z0
        mu = rng.standard_normal(ev_o.n_constraints)
        out = run_all(ev, po, Z, mu, sigma=0.7, hessian=True)
        errs = {"f": rel_err(out["f"], ev_o.eval_objective(Z)), "grad": rel_err(out["grad"], ev_o.eval_objective_gradient(Z)),
                "cons": rel_err(out["cons"], ev_o.eval_constraint(Z)), "jac": rel_err(out["jac"], ev_o.eval_constraint_jacobian(Z)),
                "hess": rel_err(out["hess"], ev_o.eval_hessian_lagrangian(Z, 0.7, mu))}
        w = rng.standard_normal(po.n_vars)
        y = np.full(ev_o.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, Z, w)
        errs["Jw"] = rel_err(y, ev_o.eval_constraint_jacobian_product(Z, w))
        wt = rng.standard_normal(ev_o.n_constraints)
        y = np.full(po.n_vars, np.nan); ev.eval_constraint_jacobian_transpose_product(y, Z, wt)
        errs["JTw"] = rel_err(y, ev_o.eval_constraint_jacobian_transpose_product(Z, wt))
        print(tag, errs, ev.last_stats())
        for k, v in errs.items():
            assert v <= (TOL_H if k == "hess" else TOL), (tag, k, v)
    finally:
        ev.close()


@pytest.mark.parametrize("n,P,N", [(40, 3, 9), (64, 2, 12), (96, 3, 8), (128, 4, 6)])
def test_callbacks_match_the_oracle(n, P, N):
    pe = multi_ket(n, P, N, seed=n + P)
    check_against_oracle(pe, [(0, P, 1)] * P + [(P, 1, 0)], f"multi-ket {n} x {P}")


def test_members_separated_by_a_derivative_integrator_match_the_oracle():
    pe = multi_ket(72, 3, 7, seed=5, derivative_between=True)
    check_against_oracle(pe, [(0, 3, 1), (1, 1, 0), (0, 3, 1), (0, 3, 1)], "multi-ket 72 x 3, derivative in between")


def test_a_fourth_integrator_with_other_generators_matches_the_oracle():
    pe = multi_ket(48, 3, 8, seed=6, extra_ket=True)
    check_against_oracle(pe, [(0, 3, 1)] * 3 + [(3, 1, 0), (4, 1, 0)], "multi-ket 48 x 3 + one of its own")


def device_jacobian(ev, Z, out=None):
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    dZ = torch.from_numpy(np.ascontiguousarray(Z)).to(dev)
    J = torch.full((ev.shard.jac_len,), float("nan"), dtype=torch.float64, device=dev) if out is None else out
    ev.eval_jacobian_dev(dZ.data_ptr(), J.data_ptr(), st)
    torch.cuda.synchronize()
    ev.last_stats()  # surfaces a deferred error of the asynchronous call
    return J


@pytest.mark.parametrize("n,P,N", [(40, 3, 9), (128, 3, 7)])
def test_followers_blocks_are_the_leaders_bits(n, P, N):
    import torch
    pe = multi_ket(n, P, N, seed=8)
    Z = pe.trajectory.vec()
    a, d = dto_amd.Evaluator(pe, shared_generators=True), dto_amd.Evaluator(pe)
    try:
        Ja, Jd = device_jacobian(a, Z), device_jacobian(d, Z)
        idx = [torch.from_numpy(e_block_index(pe, a, i)).to(Ja.device) for i in range(P)]
        lead = Ja[idx[0]]
        assert bool(torch.isfinite(lead).all()) and float(lead.abs().max()) > 0.0
        for i in range(P):
            assert torch.equal(Ja[idx[i]], lead), i               # the copies
            assert torch.equal(Jd[idx[i]], lead), i               # ... and what a chain of its own gives the same integrator
    finally:
        a.close(); d.close()


@pytest.mark.parametrize("n,P,N", [(64, 3, 10), (128, 3, 7)])
@pytest.mark.parametrize("overlap", [0, 1])
def test_deterministic_jacobian_is_the_unflagged_handles_bit_for_bit(n, P, N, overlap):
    import torch
    pe = multi_ket(n, P, N, seed=9)
    Z = pe.trajectory.vec()
    a, d = dto_amd.Evaluator(pe, shared_generators=True), dto_amd.Evaluator(pe)
    try:
        for e in (a, d):
            e.set_option("deterministic", 1)
            e.set_option("overlap_sweep", overlap)
        Ja, Jd = device_jacobian(a, Z), device_jacobian(d, Z)
        assert torch.equal(Ja, Jd), int((Ja != Jd).sum())
    finally:
        a.close(); d.close()


@pytest.mark.parametrize("n,P,N", [(64, 3, 10), (128, 3, 7), (192, 2, 6)])
def test_chains_that_square_are_shared_bit_for_bit(n, P, N):
    """Generators with the norms of the scaling benchmark (scale = 1) and a timestep of 0.3: above 64 states the propagators need
    squarings, so -E_k leaves the chain through the last squaring's store instead of the polynomial product's (at 64 states the
    one-launch chain decides per interval)."""
    import torch
    pe = multi_ket(n, P, N, seed=18, scale=1.0, dt=0.3)
    Z = pe.trajectory.vec()
    a, d = dto_amd.Evaluator(pe, shared_generators=True), dto_amd.Evaluator(pe)
    try:
        for e in (a, d):
            e.set_option("deterministic", 1)
        Ja, Jd = device_jacobian(a, Z), device_jacobian(d, Z)
        assert n <= 64 or a.last_stats()[0] >= 1, a.last_stats()
        assert torch.equal(Ja, Jd), int((Ja != Jd).sum())
        idx = [torch.from_numpy(e_block_index(pe, a, i)).to(Ja.device) for i in range(P)]
        for i in range(1, P):
            assert torch.equal(Ja[idx[i]], Ja[idx[0]]), i
        po = to_oracle(pe)
        assert rel_err(Ja.cpu().numpy(), O.OracleEvaluator(po).eval_constraint_jacobian(po.Z0)) <= TOL
    finally:
        a.close(); d.close()


def chain_counts(ev, Z):
    ev.set_option("overlap_sweep", 0)
    ev.profile_enable(True)
    ev.profile_reset()
    device_jacobian(ev, Z)
    out = {name: ev.profile_get(name) for name in ("bgemm", "basis", "chain64", "share")}
    ev.profile_enable(False)
    return out


@pytest.mark.parametrize("n,P,N", [(48, 3, 9), (64, 4, 8), (128, 3, 7)])
def test_the_chain_runs_once_per_group(n, P, N):
    """The test that fails without the feature: the launch counts of the chain's categories are those of the one-ket problem
    (same generators, controls and timestep), 1 / P of the unflagged handle's, and the copy moved P - 1 blocks per interval."""
    pe, one = multi_ket(n, P, N, seed=10), multi_ket(n, 1, N, seed=10)
    assert np.array_equal(pe.integrators[0].G, one.integrators[0].G)
    assert np.array_equal(pe.trajectory.data[pe.integrators[0].u_off:][:2], one.trajectory.data[one.integrators[0].u_off:][:2])
    a, d, s = dto_amd.Evaluator(pe, shared_generators=True), dto_amd.Evaluator(pe), dto_amd.Evaluator(one)
    try:
        ca, cd, cs = chain_counts(a, pe.trajectory.vec()), chain_counts(d, pe.trajectory.vec()), chain_counts(s, one.trajectory.vec())
        print({k: (ca[k][1], cd[k][1], cs[k][1]) for k in ca})
        for name in ("bgemm", "basis", "chain64"):
            assert ca[name][1] == cs[name][1], (name, ca[name], cs[name])
            assert cd[name][1] == P * ca[name][1], (name, cd[name], ca[name])
        assert ca["bgemm"][1] >= 1
        if n <= 64:
            assert ca["chain64"][1] == 1
        assert ca["share"][1] >= 1 and ca["share"][2] == 8.0 * (P - 1) * (N - 1) * n * n, ca["share"]
        assert cd["share"][1] == 0 and cs["share"][1] == 0
    finally:
        a.close(); d.close(); s.close()


def test_a_shard_is_a_slice_of_the_whole():
    """Knot-range shards: bit for bit the unflagged handle's shard (option deterministic), and the values of the whole
    trajectory's slice (a shard's sweep groups its intervals by its own count: the oracle's tolerance)."""
    import torch
    pe = multi_ket(96, 3, 12, seed=11)
    Z = pe.trajectory.vec()
    whole = dto_amd.Evaluator(pe, shared_generators=True)
    try:
        Jw = device_jacobian(whole, Z).cpu().numpy()
        for lo, hi in ((1, 5), (4, 9), (8, 12)):
            ev, plain = (dto_amd.Evaluator(pe, shared_generators=f, k_lo=lo, k_hi=hi) for f in (True, False))
            try:
                assert ev.integrator_share(1) == (0, 3, 1)
                for e in (ev, plain):
                    e.set_option("deterministic", 1)
                J, Jp = device_jacobian(ev, Z), device_jacobian(plain, Z)
                assert torch.equal(J, Jp), (lo, hi, int((J != Jp).sum()))
                s = ev.shard
                assert rel_err(J.cpu().numpy(), Jw[s.jac_lo:s.jac_lo + s.jac_len]) <= TOL, (lo, hi)
            finally:
                ev.close(); plain.close()
    finally:
        whole.close()


def test_chunks_of_the_chain_are_each_followed_by_their_copy():
    """chain_chunk = 8 on 25 intervals: four chunks, a copy behind each.  Bit for bit the unflagged handle's Jacobian in the same
    chunks, the followers' blocks the leader's bits, and the values of the call in one chunk (to the oracle's tolerance: with
    fewer intervals per launch the chain's launches may take another tile shape).  The host-pointer Jacobian of the chunked group,
    host_xfer on and off: the device Jacobian's bits."""
    import torch
    pe = multi_ket(128, 3, 26, seed=12)
    Z = pe.trajectory.vec()
    one, c, d = (dto_amd.Evaluator(pe, shared_generators=f) for f in (True, True, False))
    try:
        for e in (one, c, d):
            e.set_option("deterministic", 1)
        for e in (c, d):
            e.set_option("chain_chunk", 8)
        c.profile_enable(True)
        c.profile_reset()
        J1, Jc, Jd = device_jacobian(one, Z), device_jacobian(c, Z), device_jacobian(d, Z)
        assert c.profile_get("share")[1] >= 3
        assert torch.equal(Jc, Jd), int((Jc != Jd).sum())
        idx = [torch.from_numpy(e_block_index(pe, c, i)).to(Jc.device) for i in range(3)]
        assert torch.equal(Jc[idx[1]], Jc[idx[0]]) and torch.equal(Jc[idx[2]], Jc[idx[0]])
        assert rel_err(Jc.cpu().numpy(), J1.cpu().numpy()) <= TOL
        # the host-pointer Jacobian of the chunked group -- the entry point that owns the other per-chunk callback, here on a chain
        # whose chunks the group's copy follows -- with the run-wise hand-over and with the whole-slab copy: into garbage, the device
        # Jacobian's bits either way
        # (a handle each: the option is fixed at a handle's first host-pointer call)
        for on in (1, 0):
            hp = dto_amd.Evaluator(pe, shared_generators=True)
            try:
                for name, value in (("deterministic", 1), ("chain_chunk", 8), ("host_xfer", on)):
                    hp.set_option(name, value)
                Jh = np.full(hp.n_jacobian_entries, np.nan)
                hp.eval_constraint_jacobian(Jh, Z)
            finally:
                hp.close()
            differ = int((Jh.view(np.uint64) != Jc.cpu().numpy().view(np.uint64)).sum())
            print("host_xfer", on, "entries that differ from the device Jacobian:", differ)
            assert differ == 0
    finally:
        one.close(); c.close(); d.close()


def test_bound_output_keeps_a_poisoned_constant_and_tracks_the_point():
    import torch
    from dto_amd import capi
    pe = multi_ket(64, 3, 9, seed=13)
    dev = torch.device("cuda", 0)
    ev, ref = dto_amd.Evaluator(pe, shared_generators=True), dto_amd.Evaluator(pe, shared_generators=True)
    try:
        rng = np.random.default_rng(0)
        Z0 = pe.trajectory.vec()
        Zs = [Z0 + 0.05 * k * rng.standard_normal(Z0.size) for k in range(3)]
        want = [device_jacobian(ref, Z) for Z in Zs]
        varies = (want[0] != want[1]) | (want[0] != want[2])
        n = ref.shard.jac_len
        assert 0 < int(varies.sum()) < n
        buf = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        ev.bind_output_dev(capi.VECTOR_JACOBIAN, buf.data_ptr())
        for k in (0, 1, 2, 0):
            device_jacobian(ev, Zs[k], out=buf)
            assert torch.equal(buf, want[k]), (k, int((buf != want[k]).sum()))
            buf[varies] = float("nan")        # the followers' -E_k blocks among them: they are variable runs
        # a structural zero marked after priming survives the next call: the call did not rewrite it
        rows, cols = ev.jacobian_structure()
        z, du_off = pe.trajectory.dim, pe.trajectory.components["du"][0]
        pos = int(np.nonzero((cols - 1 == z + du_off) & (rows - 1 == 64))[0][0])   # a du column, a row of the first ket's second interval
        assert want[0][pos] == 0.0 and want[1][pos] == 0.0
        device_jacobian(ev, Zs[0], out=buf)
        buf[pos] = 7.0
        device_jacobian(ev, Zs[1], out=buf)
        assert buf[pos] == 7.0
        buf[pos] = 0.0
        assert torch.equal(buf, want[1])
        ev.bind_output_dev(capi.VECTOR_JACOBIAN, 0)
    finally:
        ev.close(); ref.close()


@pytest.mark.parametrize("n,N", [(64, 9), (128, 7)])
def test_host_pointer_jacobian_is_the_device_callbacks(n, N):
    pe = multi_ket(n, 3, N, seed=14)
    Z = pe.trajectory.vec()
    ev = dto_amd.Evaluator(pe, shared_generators=True)
    try:
        ev.set_option("deterministic", 1)   # (the two entry-point families then take the same chunks and sweep shapes)
        Jd = device_jacobian(ev, Z).cpu().numpy()
        Jh = np.full(ev.shard.jac_len, np.nan)
        ev.eval_constraint_jacobian(Jh, Z)
        assert np.array_equal(Jh, Jd), int((Jh != Jd).sum())
    finally:
        ev.close()


def test_repeated_calls_are_bit_identical():
    import torch
    pe = multi_ket(96, 3, 9, seed=15)
    Z = pe.trajectory.vec()
    ev = dto_amd.Evaluator(pe, shared_generators=True)
    try:
        runs = [device_jacobian(ev, Z) for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    finally:
        ev.close()


def test_reuse_forward_sweep_serves_the_followers():
    """g, J, H at one point with the option on: the followers' step plans and cached sweeps are recorded like the leader's."""
    pe = multi_ket(64, 3, 9, seed=16)
    po = to_oracle(pe)
    ev_o = O.OracleEvaluator(po)
    ev = dto_amd.Evaluator(pe, shared_generators=True)
    try:
        ev.set_option("reuse_forward_sweep", 1)
        Z = po.Z0
        mu = np.random.default_rng(1).standard_normal(ev_o.n_constraints)
        for _ in range(2):
            j = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(j, Z)
            c = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(c, Z)
            h = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(h, Z, 0.7, mu)
            assert rel_err(j, ev_o.eval_constraint_jacobian(Z)) <= TOL
            assert rel_err(c, ev_o.eval_constraint(Z)) <= TOL
            assert rel_err(h, ev_o.eval_hessian_lagrangian(Z, 0.7, mu)) <= TOL_H
    finally:
        ev.close()


def test_an_inactive_group_gives_the_unflagged_handles_bits():
    import torch
    pe = multi_ket(16, 3, 9, seed=17)
    Z = pe.trajectory.vec()
    a, d = dto_amd.Evaluator(pe, shared_generators=True), dto_amd.Evaluator(pe)
    try:
        assert [a.integrator_share(i) for i in range(3)] == [(0, 3, 0)] * 3
        mu = np.random.default_rng(3).standard_normal(a.n_constraints)
        oa, od = run_all(a, None, Z, mu, 0.7), run_all(d, None, Z, mu, 0.7)
        for k in oa:
            assert np.array_equal(oa[k], od[k]), k
        assert torch.equal(device_jacobian(a, Z), device_jacobian(d, Z))
        a.profile_enable(True); a.profile_reset()
        device_jacobian(a, Z)
        assert a.profile_get("share")[1] == 0
    finally:
        a.close(); d.close()
