"""GPU: TimeDependentBilinearIntegrators of one system share one propagation (DTO_FLAG_SHARED_GENERATORS on the time-dependent
kind, the group form of k_tdb_mfma in csrc/dto_tdb_mfma.hip).

Reference: tests/tdb_large_cases.reference on tests/tdb_share_cases.py's problems (P O.TimeDependentBilinearIntegrators on one
family); bars 1e-10 relative for values and Jacobian, 1e-8 for the Hessian, as tests/test_gpu_time_dependent_large.py.  Against the
unflagged handle every output is compared bit for bit.  Shapes are the smallest at which the path can go wrong: N = 3 (two
intervals), N = 5 where sharded."""
import numpy as np
import pytest

import tdb_share_cases as S
from helpers import rel_err, to_engine

pytestmark = pytest.mark.gpu


def _all(ev, Z, mu, sigma=0.6):
    g = np.empty(ev.shard.cons_len); ev.eval_constraint(g, Z)
    j = np.empty(ev.shard.jac_len); ev.eval_constraint_jacobian(j, Z)
    h = np.empty(ev.shard.hess_len); ev.eval_hessian_lagrangian(h, Z, sigma, mu)
    return g, j, h


def _products(ev, Z, mu, seed=5, sigma=0.6):
    rng = np.random.default_rng(seed)
    w, wt, v = rng.standard_normal(ev.n_variables), rng.standard_normal(ev.n_constraints), rng.standard_normal(ev.n_variables)
    y = np.empty(ev.n_constraints); ev.eval_constraint_jacobian_product(y, Z, w)
    yt = np.empty(ev.n_variables); ev.eval_constraint_jacobian_transpose_product(yt, Z, wt)
    yh = np.empty(ev.n_variables); ev.eval_hessian_lagrangian_product(yh, Z, v, sigma, mu)
    return y, yt, yh


def _launches(ev, Z, mu, sigma=0.6, name="tdb_mfma"):
    """Launches under profile name `name` of one eval_constraint, one Jacobian and one Hessian call."""
    out = []
    ev.profile_enable(True)
    for call in (lambda: ev.eval_constraint(np.empty(ev.shard.cons_len), Z), lambda: ev.eval_constraint_jacobian(np.empty(ev.shard.jac_len), Z),
                 lambda: ev.eval_hessian_lagrangian(np.empty(ev.shard.hess_len), Z, sigma, mu)):
        ev.profile_reset()
        call()
        out.append(ev.profile_get(name)[1])
    ev.profile_enable(False)
    return out


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: "%dx%d" % c[:2])
def test_group_launch_matches_the_reference_and_the_unflagged_handle_bit_for_bit(case):
    import dto_amd
    n, P = case[:2]
    po = S.case(*case)
    ev_r, mu, g_r, j_r, h_r = S.reference(po, case)
    p = to_engine(po)
    ev, plain = dto_amd.Evaluator(p, shared_generators=True), dto_amd.Evaluator(p)
    try:
        tdb = [i for i, it in enumerate(po.integrators) if it.__class__.__name__ == "TimeDependentBilinearIntegrator"]
        assert [ev.integrator_share(i) for i in tdb] == [(tdb[0], P, 1)] * P
        r, c = ev.jacobian_structure()
        assert np.array_equal(r, ev_r.jacobian_structure1()[0]) and np.array_equal(c, ev_r.jacobian_structure1()[1])
        r, c = ev.hessian_lagrangian_structure()
        assert np.array_equal(r, ev_r.hessian_structure1()[0]) and np.array_equal(c, ev_r.hessian_structure1()[1])
        g, j, h = _all(ev, po.Z0, mu)
        errs = (rel_err(g, g_r), rel_err(j, j_r), rel_err(h, h_r))
        print("tdb group vs reference", case, errs)
        assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-8, errs
        g0, j0, h0 = _all(plain, po.Z0, mu)
        assert np.array_equal(g, g0) and np.array_equal(j, j0) and np.array_equal(h, h0), \
            (int((g != g0).sum()), int((j != j0).sum()), int((h != h0).sum()))
        for a, b in zip(_products(ev, po.Z0, mu), _products(plain, po.Z0, mu)):
            assert np.array_equal(a, b)
        assert _launches(ev, po.Z0, mu) == [1, 1, 1] and _launches(plain, po.Z0, mu) == [P, P, P]
    finally:
        ev.close(); plain.close()


def test_launches_follow_tdb_share_members_and_the_bits_do_not():
    import dto_amd
    case = S.CASES[1]   # 72 states, three kets
    po = S.case(*case)
    mu = S.reference(po, case)[1]
    p = to_engine(po)
    ev = dto_amd.Evaluator(p, shared_generators=True)
    try:
        ref = _all(ev, po.Z0, mu)
        assert _launches(ev, po.Z0, mu) == [1, 1, 1]
        for members, want in ((2, 2), (1, 3), (3, 1)):
            ev.set_option("tdb_share_members", members)
            assert _launches(ev, po.Z0, mu) == [want] * 3, members
            for a, b in zip(_all(ev, po.Z0, mu), ref):
                assert np.array_equal(a, b), members
        with pytest.raises(Exception, match="tdb_share_members"):
            ev.set_option("tdb_share_members", 4)
    finally:
        ev.close()


def test_a_members_bits_do_not_depend_on_the_group():
    """Member 0's rows of g, J and its blocks of H are the same in a group of two and a group of three: the two-ket problem is the
    three-ket problem's first two kets with the third integrator on a family of its own (same components, same point)."""
    import dto_amd
    n = 72
    three = S.problem(n, 3, m=1)
    other = S.family(n, 1, 2, seed=9)
    two = S.problem(n, 3, m=1, members=[{}, {}, {"G": other[0], "mods": other[1]}])
    assert np.array_equal(three.Z0, two.Z0)
    a, b = dto_amd.Evaluator(to_engine(three), shared_generators=True), dto_amd.Evaluator(to_engine(two), shared_generators=True)
    try:
        assert a.integrator_share(0) == (0, 3, 1) and b.integrator_share(0) == (0, 2, 1) and b.integrator_share(2) == (2, 1, 0)
        mu = np.random.default_rng(4).standard_normal(a.n_constraints)
        mu[2 * 2 * n:3 * 2 * n] = 0.0           # the third integrator's rows stay out of the Hessian: its family differs
        ga, ja, ha = _all(a, three.Z0, mu)
        gb, jb, hb = _all(b, two.Z0, mu)
        K = 2
        assert np.array_equal(ga[:2 * K * n], gb[:2 * K * n])
        r, c = a.jacobian_structure()
        rows = r <= 2 * K * n                    # the rows of members 0 and 1
        assert np.array_equal(ja[rows], jb[rows])
        assert np.array_equal(ha, hb)
    finally:
        a.close(); b.close()


def test_sharded_slabs_tile_the_unsharded_vectors_bit_for_bit():
    import dto_amd
    po = S.problem(72, 2, N=5, derivative_between=True)
    p = to_engine(po)
    full = dto_amd.Evaluator(p, shared_generators=True)
    mu = np.random.default_rng(2).standard_normal(full.n_constraints)
    g, j, h = _all(full, po.Z0, mu)
    full.close()
    for world in (2, 3):
        gj, gh, gg = np.full_like(j, np.nan), np.full_like(h, np.nan), np.full_like(g, np.nan)
        for lo, hi in dto_amd.distributed.shard_ranges(5, world):
            e = dto_amd.Evaluator(p, k_lo=lo, k_hi=hi, shared_generators=True)
            assert e.integrator_share(0) == (0, 2, 1)
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


def test_outputs_are_fully_written_and_stay_inside_the_owned_slab():
    """The middle shard of three, a DerivativeIntegrator between the members: device buffers pre-filled with NaN and with guard
    zones on both sides hold no NaN inside and only NaN outside."""
    import torch
    import dto_amd
    po = S.problem(72, 2, N=5, derivative_between=True)
    ev = dto_amd.Evaluator(to_engine(po), k_lo=3, k_hi=4, shared_generators=True)
    try:
        assert ev.integrator_share(2) == (0, 2, 1)
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


def test_an_inactive_group_is_evaluated_as_without_the_flag():
    """24 states (k_tdb): grouped, inactive, bit for bit the unflagged handle and no k_tdb_mfma launch.  The structured path
    (k_tdb_kron, 72 states as six 12 x 12 blocks), whose launches the profile counts: one per member, flagged or not."""
    import dto_amd
    po = S.problem(24, 2)
    p = to_engine(po)
    ev, plain = dto_amd.Evaluator(p, shared_generators=True), dto_amd.Evaluator(p)
    try:
        assert ev.integrator_share(1) == (0, 2, 0)
        mu = np.random.default_rng(3).standard_normal(ev.n_constraints)
        for a, b in zip(_all(ev, po.Z0, mu), _all(plain, po.Z0, mu)):
            assert np.array_equal(a, b)
        assert _launches(ev, po.Z0, mu) == [0, 0, 0]
    finally:
        ev.close(); plain.close()
    rng = np.random.default_rng(4)
    kron = lambda B: np.stack([np.kron(np.eye(6), Bj) for Bj in B]) / 3.0
    fam = {"G": kron(rng.standard_normal((3, 12, 12))), "mods": [("cos", 1.7, kron(rng.standard_normal((3, 12, 12))))]}
    po = S.problem(72, 2, members=[fam, fam])
    p = to_engine(po)
    ev, plain = dto_amd.Evaluator(p, shared_generators=True, block_generators=True), dto_amd.Evaluator(p, block_generators=True)
    try:
        assert ev.integrator_share(1) == (0, 2, 0) and ev.integrator_blocks(1) == (12, 6, 1)
        mu = np.random.default_rng(3).standard_normal(ev.n_constraints)
        for a, b in zip(_all(ev, po.Z0, mu), _all(plain, po.Z0, mu)):
            assert np.array_equal(a, b)
        assert _launches(ev, po.Z0, mu, name="tdb_kron") == [2, 2, 2] and _launches(ev, po.Z0, mu) == [0, 0, 0]
    finally:
        ev.close(); plain.close()
