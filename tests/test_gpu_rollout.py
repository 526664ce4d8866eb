"""GPU: the open-loop rollout X_{k+1} = E_k(Z) X_k (dto_rollout / dto_rollout_dev, csrc/dto_rollout.hip).

Reference, independent of the engine and of the tree: for a bilinear integrator scipy.linalg.expm(dt_k (G_0 + sum_j u_kj G_j)) @ X_k,
step by step in NumPy; for the time-dependent kind the oracle's own fixed-step map, -integ.f(zz) with x_k set to the rolled state and
x_{k+1} set to zero.  Bar: rel_err(X, X_ref) <= helpers.TOL max(1, K / 16) -- every E_k entry is held to TOL by the existing tests
(measured at <= 5e-14) and with ||E_k||_2 = 1 K steps add at most K such errors.  Outputs are pre-filled with NaN (Evaluator.rollout
does, the device tests do it themselves) so that a missing writer shows.  The largest error seen over all cases is in DESIGN 4.23."""
import functools

import numpy as np
import pytest
import scipy.linalg

import dto_amd
import dto_oracle as O
import scan_cases as S
from helpers import TOL, rel_err, to_engine
from multi_ket_cases import multi_ket
from test_gpu_block_generators import kron_problem
from test_gpu_jacobian_products import case as products_case
from test_gpu_scan_accuracy_budget import open_case

pytestmark = pytest.mark.gpu

STEPS = (1e-4, 0.1, 1.0, 3.0)   # the large ones run the chain's squarings, the small ones its no-squaring store


def bar(K):
    return TOL * max(1.0, K / 16.0)


def with_steps(p, seed):
    """dt drawn from STEPS per knot"""
    Zk = p.Z0.reshape(p.N, p.z).copy()
    Zk[:, p.dt_idx] = np.random.default_rng(seed).choice(STEPS, p.N)
    p.Z0 = Zk.reshape(-1).copy()
    return p


def scaled(N, n, m=2, seed=0):
    """orthogonal propagators: skew-symmetric generators"""
    return with_steps(O.make_scaled_problem(N, n, m, seed=200 + n + N + seed, skew=True), seed=n + N)


def reference(it, Z, N, z, dt_idx, X0):
    """(N, n_cols, x_dim): the integrator's dynamics applied step by step.  `it`: an oracle or host-mirror BilinearIntegrator, or the
    oracle's TimeDependentBilinearIntegrator."""
    Zk = np.asarray(Z)[:N * z].reshape(N, z)
    n = it.x_dim
    X = np.empty((N,) + X0.shape)
    X[0] = X0
    for k in range(N - 1):
        if isinstance(it, O.TimeDependentBilinearIntegrator):
            zz = np.tile(np.concatenate([Zk[k], Zk[k + 1]]), (X0.shape[0], 1))
            zz[:, it.x_off:it.x_off + n] = X[k]
            zz[:, z + it.x_off:z + it.x_off + n] = 0.0
            X[k + 1] = -it.f(zz)
        else:
            G = np.asarray(it.G)
            A = G[0] + np.einsum("j,jrc->rc", Zk[k, it.u_off:it.u_off + it.u_dim], G[1:])
            X[k + 1] = X[k] @ scipy.linalg.expm(Zk[k, dt_idx] * A).T
    return X


def start_states(n, n_cols, seed=7):
    return np.random.default_rng(seed).standard_normal((n_cols, n))


@functools.lru_cache(maxsize=None)
def scaled_case(N, n, n_cols):
    """problem, point, start states and reference: computed once, shared, never written"""
    p = scaled(N, n)
    X0 = start_states(n, n_cols)
    ref = reference(p.integrators[0], p.Z0, p.N, p.z, p.dt_idx, X0)
    for a in (p.Z0, X0, ref):
        a.setflags(write=False)
    return p, X0, ref


def check(ev, Z, X0, ref, K, tag, integrator=0):
    X = ev.rollout(Z, integrator=integrator, X0=X0)
    assert X.shape == ref.shape
    assert np.array_equal(X[0], np.atleast_2d(X0)), "knot 1 is a copy of X0"
    err = rel_err(X, ref)
    print(tag, "K", K, "rel_err", err, "bar", bar(K), "max |x|", float(np.max(np.abs(ref))))
    assert err <= bar(K), (tag, err)   # (NaN, a missing writer, fails the comparison)
    return X


# ---------------------------------------------------------------------------------------------------------------- paths
@pytest.mark.parametrize("n,N", [(5, 4), (40, 6), (70, 12), (130, 5), (256, 5)],
                         ids=["k_small", "k_chain64", "general_npad128", "general_npad192", "general_ring256"])
def test_bilinear_paths(n, N):
    p, X0, ref = scaled_case(N, n, 3)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        check(ev, p.Z0, X0, ref, N - 1, "n=%d" % n)
    finally:
        ev.close()


def test_general_path_flag_on_a_small_integrator():
    p, X0, ref = scaled_case(4, 5, 3)
    ev = dto_amd.Evaluator(to_engine(p), general_path_only=True)
    try:
        check(ev, p.Z0, X0, ref, 3, "general_path_only n=5")
    finally:
        ev.close()


def test_structured_path():
    p = kron_problem(16, 4, 2, 5, seed=3)
    ev = dto_amd.Evaluator(to_engine(p), block_generators=True)
    try:
        assert ev.integrator_blocks(0) == (16, 4, 1)
        X0 = start_states(64, 3)
        check(ev, p.Z0, X0, reference(p.integrators[0], p.Z0, p.N, p.z, p.dt_idx, X0), p.N - 1, "structured 16x4")
    finally:
        ev.close()


@pytest.mark.parametrize("n,N", [(4, 6), (72, 5)], ids=["k_tdb", "k_tdb_mfma"])
def test_time_dependent_paths(n, N):
    p = O.make_tdb_problem(N=N, n=n, m=2, substeps=16)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        X0 = start_states(n, 3)
        check(ev, p.Z0, X0, reference(p.integrators[0], p.Z0, p.N, p.z, p.dt_idx, X0), N - 1, "tdb n=%d" % n)
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------------- tree shapes
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 9, 37, 64, 65])
def test_tree_shapes(K):
    """no level; one level; an identity leaf; the root delivers the last knot; mixed; dead items in several levels; 2^L and 2^L + 1"""
    p, X0, ref = scaled_case(K + 1, 12, 2)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        X = check(ev, p.Z0, X0, ref, K, "tree K=%d" % K)
        F = ev.rollout(p.Z0, X0=X0, all_knots=False)
        assert F.shape == (2, 12) and np.array_equal(F, X[-1]), "FINAL is the last block of ALL, bit for bit"
    finally:
        ev.close()


# -------------------------------------------------------------------------------------------------------------- columns
@pytest.fixture(scope="module")
def ev40():
    p, _, _ = scaled_case(6, 40, 40)
    ev = dto_amd.Evaluator(to_engine(p))
    yield ev
    ev.close()


@pytest.mark.parametrize("n_cols", [1, 16, 17, 40])
def test_column_counts(ev40, n_cols):
    """one column, a whole column tile, one column past it, the full basis"""
    p, X0, ref = scaled_case(6, 40, 40)
    check(ev40, p.Z0, X0[:n_cols], ref[:, :n_cols], 5, "n_cols=%d" % n_cols)


def test_full_basis_gives_the_cumulative_propagator(ev40):
    p = scaled_case(6, 40, 40)[0]
    I = np.eye(40)
    prod = reference(p.integrators[0], p.Z0, p.N, p.z, p.dt_idx, I)[-1].T   # E_K ... E_1 (row c of the rollout is column c)
    U = ev40.rollout(p.Z0, X0=I, all_knots=False).T
    err = rel_err(U, prod)
    print("cumulative propagator", err, "orthogonality", float(np.max(np.abs(U.T @ U - I))))
    assert err <= bar(5)


def test_a_column_has_the_same_bits_alone_and_among_others(ev40):
    p, X0, _ = scaled_case(6, 40, 40)
    alone = ev40.rollout(p.Z0, X0=X0[0])
    for n_cols in (17, 40):
        among = ev40.rollout(p.Z0, X0=X0[:n_cols])
        assert np.array_equal(among[:, 0], alone[:, 0]), n_cols


def test_the_64_column_tile_keeps_the_bits_of_the_16_column_tile():
    """49 columns and more run the descent on 64-column tiles: the same K order, so the same bits"""
    p, _, _ = scaled_case(12, 70, 3)
    X0 = start_states(70, 70, seed=9)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        wide = check(ev, p.Z0, X0, reference(p.integrators[0], p.Z0, p.N, p.z, p.dt_idx, X0), 11, "n_cols=70 of 70")
        for c in (0, 48, 69):
            assert np.array_equal(ev.rollout(p.Z0, X0=X0[c])[:, 0], wide[:, c]), c
    finally:
        ev.close()


def test_no_X0_takes_the_state_of_knot_1(ev40):
    p = scaled_case(6, 40, 40)[0]
    x1 = p.Z0[:40].copy()
    assert np.array_equal(ev40.rollout(p.Z0), ev40.rollout(p.Z0, X0=x1))
    Z = p.Z0.copy()
    Z.reshape(p.N, p.z)[1:, :40] = np.random.default_rng(4).standard_normal((p.N - 1, 40))   # the other knots' states do not matter
    assert np.array_equal(ev40.rollout(Z), ev40.rollout(p.Z0, X0=x1))


# ------------------------------------------------------------------------------------------------ modes and determinism
WHERE = ["n40"] + list(S.CASES)


@pytest.fixture(scope="module")
def places(ev40):
    """where -> (handle, oracle problem, Z, integrator, up to 40 start states): the 40-state handle, and one handle per case of
    tests/scan_cases.py at its fixture's point (every path the rollout serves; tdbhp_n72: the follower of the group of two),
    opened on first use and closed with the module."""
    opened = {}

    def get(where):
        if where == "n40":
            p, X0, _ = scaled_case(6, 40, 40)
            return ev40, p, p.Z0, 0, X0
        if where not in opened:
            ev, Z, q, p, fix = open_case(where)
            n = fix["X0"].shape[1]
            opened[where] = (ev, p, Z, q, S.more_columns(where, min(n, 40), fix["X0"], fix["B"])[0])
        return opened[where]

    yield get
    for place in opened.values():
        place[0].close()


@pytest.mark.parametrize("where", WHERE)
def test_final_mode_and_repeated_calls_are_bit_identical(places, where):
    ev, p, Z, q, X0 = places(where)
    a = ev.rollout(Z, integrator=q, X0=X0[:17])
    b = ev.rollout(Z, integrator=q, X0=X0[:17])
    f = ev.rollout(Z, integrator=q, X0=X0[:17], all_knots=False)
    assert np.array_equal(a, b) and np.array_equal(f, a[-1]) and not np.isnan(a).any()


@pytest.mark.parametrize("where", WHERE)
def test_device_pointer_form_gives_the_bits_of_the_host_pointer_form(places, where):
    import torch
    ev, p, Z, q, X0 = places(where)
    n = X0.shape[1]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    dZ = torch.from_numpy(np.array(Z)).to(dev)
    for n_cols, all_knots in ((17, True), (17, False), (1, True)):
        x0 = np.array(X0[:n_cols])
        n_cols = x0.shape[0]      # (fewer than 17 states: every one of them)
        dX0 = torch.from_numpy(x0).to(dev)
        shape = (p.N, n_cols, n) if all_knots else (n_cols, n)
        dX = torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        ev.rollout_dev(dZ.data_ptr(), dX0.data_ptr(), n_cols, dX.data_ptr(), integrator=q, all_knots=all_knots, stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(dX.cpu().numpy(), ev.rollout(Z, integrator=q, X0=x0, all_knots=all_knots)), (n_cols, all_knots)
    dX = torch.full((p.N, 1, n), float("nan"), dtype=torch.float64, device=dev)
    ev.rollout_dev(dZ.data_ptr(), 0, 1, dX.data_ptr(), integrator=q, stream=st)   # X0 = NULL
    torch.cuda.synchronize()
    assert np.array_equal(dX.cpu().numpy(), ev.rollout(Z, integrator=q))


# --------------------------------------------------------------------------------------------------- several integrators
def test_integrators_are_named_by_their_position():
    """structured (64 states), derivative, dense (40 states) in one handle"""
    c = products_case("mixed:40")
    p = c["p"]
    ev = dto_amd.Evaluator(c["pe"], **c["kw"])
    try:
        assert ev.integrator_blocks(0)[2] == 1
        for i in (2, 0):
            it = p.integrators[i]
            X0 = start_states(it.x_dim, 3, seed=i)
            check(ev, c["Z"], X0, reference(it, c["Z"], p.N, p.z, p.dt_idx, X0), p.N - 1, "mixed integrator %d" % i, integrator=i)
        with pytest.raises(dto_amd.EngineError, match="DerivativeIntegrator"):
            ev.rollout(c["Z"], integrator=1, X0=np.ones(2))
        ev.rollout(c["Z"], integrator=2)   # the handle stays usable
    finally:
        ev.close()


def test_follower_of_a_shared_group_rolls_out_the_leaders_bits():
    pe = multi_ket(40, 2, 5)
    Z = np.ascontiguousarray(pe.trajectory.vec(), dtype=np.float64)
    traj = pe.trajectory
    ev = dto_amd.Evaluator(pe, shared_generators=True)
    try:
        assert ev.integrator_share(1) == (0, 2, 1)
        X0 = start_states(40, 3)
        ref = reference(pe.integrators[0], Z, traj.N, traj.dim, traj.components[traj.timestep][0], X0)
        lead = check(ev, Z, X0, ref, traj.N - 1, "shared leader", integrator=0)
        follow = check(ev, Z, X0, ref, traj.N - 1, "shared follower", integrator=1)
        assert np.array_equal(lead, follow)
    finally:
        ev.close()


def test_external_integrator_is_refused():
    p = O.make_external_integrator_problem()
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        ext = [i for i, it in enumerate(p.integrators) if it.kind == "external"][0]
        with pytest.raises(dto_amd.EngineError, match="evaluated on the host"):
            ev.rollout(p.Z0, integrator=ext, X0=np.ones(p.integrators[ext].x_dim))
        g = np.full(ev.n_constraints, np.nan); ev.eval_constraint(g, p.Z0)
        assert not np.isnan(g).any()
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------------- feasibility
@pytest.mark.parametrize("kind", ["bilinear_general", "time_dependent"])
def test_rolled_states_satisfy_the_dynamics_constraints(kind):
    """The scan against the sweep, which shares no code with it: with the rolled states written back into Z the integrator's
    defect rows vanish to TOL max(1, |x|)."""
    p = scaled_case(12, 70, 3)[0] if kind == "bilinear_general" else O.make_tdb_problem(N=6, n=4, m=2, substeps=16)
    it = p.integrators[0]
    n, K = it.x_dim, p.N - 1
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        X = ev.rollout(p.Z0)[:, 0]
        Z = np.array(p.Z0)
        Z[:p.N * p.z].reshape(p.N, p.z)[:, it.x_off:it.x_off + n] = X
        g = np.full(ev.n_constraints, np.nan); ev.eval_constraint(g, Z)
        rows = g[:K * n].reshape(K, n)     # the first integrator's rows come first
        worst = float(np.max(np.abs(rows) / np.maximum(1.0, np.abs(X[1:]))))
        print(kind, "largest defect / max(1, |x|)", worst)
        assert worst <= TOL
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_reason_and_leave_the_handle_usable(ev40):
    p, X0, ref = scaled_case(6, 40, 40)
    lib, dp = dto_amd.load_library(), dto_amd.capi.c_double_p
    with pytest.raises(dto_amd.EngineError, match="n_cols = 0"):
        ev40.rollout(p.Z0, X0=np.empty((0, 40)))
    with pytest.raises(dto_amd.EngineError, match="n_cols = 41"):
        ev40.rollout(p.Z0, X0=np.ones((41, 40)))
    Z, x0, out = np.array(p.Z0), np.array(X0[:1]), np.full((6, 1, 40), np.nan)
    assert lib.dto_rollout(ev40.handle, 0, Z.ctypes.data_as(dp), x0.ctypes.data_as(dp), 1, 2, out.ctypes.data_as(dp)) != 0
    assert "mode" in lib.dto_last_error(ev40.handle).decode() and np.isnan(out).all()
    assert lib.dto_rollout(ev40.handle, 0, Z.ctypes.data_as(dp), None, 2, 0, out.ctypes.data_as(dp)) != 0
    assert "X0 = NULL" in lib.dto_last_error(ev40.handle).decode()
    for bad in (-1, 2):   # the handle has two integrators
        with pytest.raises(dto_amd.EngineError, match="out of range"):
            ev40.rollout(p.Z0, integrator=bad, X0=np.ones(1))
    check(ev40, p.Z0, X0[:3], ref[:, :3], 5, "after the refusals")


def test_a_sharded_handle_is_refused():
    p = scaled_case(6, 40, 40)[0]
    ev = dto_amd.Evaluator(to_engine(p), k_lo=1, k_hi=3)
    try:
        with pytest.raises(dto_amd.EngineError, match="unsharded"):
            ev.rollout(p.Z0)
        g = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(g, p.Z0)
        assert not np.isnan(g).any()
    finally:
        ev.close()


# -------------------------------------------------------------------------------------------------------------- profile
def test_profile_category():
    import torch
    p, X0, _ = scaled_case(12, 70, 3)
    K, L = 11, 4
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        ev.set_option("overlap_sweep", 0)
        dZ = torch.from_numpy(np.array(p.Z0)).to(dev)
        dX0 = torch.from_numpy(np.array(X0)).to(dev)
        dX = torch.full((12, 3, 70), float("nan"), dtype=torch.float64, device=dev)
        dJ = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dev)
        ev.profile_enable(True); ev.profile_reset()
        ev.rollout_dev(dZ.data_ptr(), dX0.data_ptr(), 3, dX.data_ptr(), stream=st)
        torch.cuda.synchronize()
        ms, launches, flops = ev.profile_get("rollout")
        plain, every = ev.profile_get("bgemm_plain")[1], ev.profile_get("all")[1]
        print("rollout", ms, launches, flops, "bgemm_plain", plain, "all", every)
        assert launches >= 1 + L + L and ms > 0.0
        parts = [ev.profile_get("rollout_" + part) for part in ("gather", "tree", "descent")]
        print("gather, tree, descent", parts)
        assert [q[1] for q in parts[:2]] == [1, L] and parts[2][1] >= L and sum(q[1] for q in parts) == launches
        assert parts[1][2] == 2.0 * 128 ** 3 * (2 ** L - 1) and sum(q[2] for q in parts) == flops
        assert flops >= 2.0 * 128 ** 3 * (2 ** L - 1)   # the tree's products alone, padded
        ev.eval_jacobian_dev(dZ.data_ptr(), dJ.data_ptr(), st)
        torch.cuda.synchronize()
        assert ev.profile_get("rollout")[1] == launches
        # the Jacobian inside the rollout counted under its own names exactly as a Jacobian alone does; the tree's products did not
        assert ev.profile_get("bgemm_plain")[1] == 2 * plain and ev.profile_get("all")[1] == 2 * every
        ev.profile_enable(False)
    finally:
        ev.close()
