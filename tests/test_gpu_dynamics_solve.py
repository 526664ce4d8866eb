"""GPU: solves with the dynamics block (dto_dynamics_solve / dto_dynamics_solve_dev, csrc/dto_dynsolve.hip) -- the linearised rollout
Y_1 = B_1, Y_{k+1} = E_k Y_k + B_{k+1} and the costate recursion L_N = B_N, L_k = E_k' L_{k+1} + B_k.

Reference, independent of the engine and of the tree: the two recurrences in NumPy on E_k assembled once per case -- for a bilinear
integrator scipy.linalg.expm(dt_k (G_0 + sum_j u_kj G_j)), for the time-dependent kind the oracle's own fixed-step map applied to the
n basis columns.  Bar: rel_err <= helpers.TOL max(1, K / 16), the rollout's bar for the rollout's reason (every E_k entry is held to
TOL by the existing tests and K steps add at most K such errors).  The same cases are checked against the engine's own J v and J' w,
which share no code with the scan.  Outputs are pre-filled with NaN so that a missing writer shows.  The largest errors seen are in
DESIGN 4.25."""
import functools

import numpy as np
import pytest
import scipy.linalg

import dto_amd
import dto_oracle as O
from helpers import TOL, rel_err, to_engine
from multi_ket_cases import multi_ket
from test_gpu_block_generators import kron_problem
from test_gpu_rollout import WHERE, bar, places, scaled_case  # noqa: F401  (`places`: the module-scoped fixture, one set of handles per module)

pytestmark = pytest.mark.gpu


def propagators(it, Z, N, z, dt_idx):
    """(K, n, n): E_k of every interval.  `it`: an oracle or host-mirror BilinearIntegrator, or the oracle's
    TimeDependentBilinearIntegrator."""
    Zk = np.asarray(Z)[:N * z].reshape(N, z)
    n = it.x_dim
    E = np.empty((N - 1, n, n))
    for k in range(N - 1):
        if isinstance(it, O.TimeDependentBilinearIntegrator):
            zz = np.tile(np.concatenate([Zk[k], Zk[k + 1]]), (n, 1))
            zz[:, it.x_off:it.x_off + n] = np.eye(n)
            zz[:, z + it.x_off:z + it.x_off + n] = 0.0
            E[k] = (-it.f(zz)).T              # row c of the map's output is E_k e_c
        else:
            G = np.asarray(it.G)
            E[k] = scipy.linalg.expm(Zk[k, dt_idx] * (G[0] + np.einsum("j,jrc->rc", Zk[k, it.u_off:it.u_off + it.u_dim], G[1:])))
    return E


def recurrence(E, B, adjoint):
    """B, result: (N, n_cols, n), one column per row"""
    K = E.shape[0]
    Y = np.empty_like(B)
    if adjoint:
        Y[K] = B[K]
        for k in range(K - 1, -1, -1):
            Y[k] = Y[k + 1] @ E[k] + B[k]
    else:
        Y[0] = B[0]
        for k in range(K):
            Y[k + 1] = Y[k] @ E[k].T + B[k + 1]
    return Y


def rhs(N, n_cols, n, seed=11):
    return np.random.default_rng(seed).standard_normal((N, n_cols, n))


PATHS = {"k_small": ("bilinear", 5, 4), "k_chain64": ("bilinear", 40, 6), "general_npad128": ("bilinear", 70, 12),
         "general_npad192": ("bilinear", 130, 5), "general_ring256": ("bilinear", 256, 5), "structured_16x4": ("structured", 64, 5),
         "k_tdb": ("tdb", 4, 6), "k_tdb_mfma": ("tdb", 72, 5), "shared_follower": ("follower", 40, 5)}


@functools.lru_cache(maxsize=None)
def path_case(name):
    """engine problem, keywords, point, E_k, right-hand side and both references: computed once, shared, never written"""
    kind, n, N = PATHS[name]
    kw, integrator = {}, 0
    if kind == "follower":
        pe = multi_ket(n, 2, N)
        traj = pe.trajectory
        Z, it, z, dt_idx = np.ascontiguousarray(traj.vec(), dtype=np.float64), pe.integrators[0], traj.dim, traj.components[traj.timestep][0]
        kw, integrator = dict(shared_generators=True), 1
    else:
        if kind == "bilinear":
            p = scaled_case(N, n, 3)[0]
        elif kind == "structured":
            p, kw = kron_problem(16, 4, 2, N, seed=3), dict(block_generators=True)
        else:
            p = O.make_tdb_problem(N=N, n=n, m=2, substeps=16)
        pe, Z, it, z, dt_idx = to_engine(p), np.array(p.Z0), p.integrators[0], p.z, p.dt_idx
    E = propagators(it, Z, N, z, dt_idx)
    B = rhs(N, 3, n)
    ref = (recurrence(E, B, False), recurrence(E, B, True))
    for a in (Z, E, B) + ref:
        a.setflags(write=False)
    return dict(pe=pe, kw=kw, Z=Z, N=N, n=n, z=z, integrator=integrator, E=E, B=B, ref=ref)


def state_slots(ev, c):
    """first row of the integrator in g, and the position of its states inside a knot"""
    return ev._integrator_row0[c["integrator"]], ev._integrator_x_off[c["integrator"]]


# ------------------------------------------------------------------------------------------------- values, every path
@pytest.mark.parametrize("name", list(PATHS))
def test_values_and_the_engines_own_products_on_every_path(name):
    c = path_case(name)
    N, n, z, K = c["N"], c["n"], c["z"], c["N"] - 1
    ev = dto_amd.Evaluator(c["pe"], **c["kw"])
    try:
        if name == "shared_follower":
            assert ev.integrator_share(1) == (0, 2, 1)
        row0, x_off = state_slots(ev, c)
        Y = ev.dynamics_solve(c["Z"], c["B"], integrator=c["integrator"])
        Lam = ev.dynamics_solve(c["Z"], c["B"], integrator=c["integrator"], adjoint=True)
        assert Y.shape == Lam.shape == c["B"].shape
        errs = dict(forward=rel_err(Y, c["ref"][0]), adjoint=rel_err(Lam, c["ref"][1]))
        # the scan against the sweeps: J v with Y in the state components returns B_{k+1} in the integrator's rows; the state
        # components of J' w with w holding Lam_{k+1} are B_k at knots 2 .. N
        Jv, JTw = np.empty((K, 3, n)), np.empty((K, 3, n))
        for col in range(3):
            v = np.zeros(ev.n_variables)
            v[:N * z].reshape(N, z)[:, x_off:x_off + n] = Y[:, col]
            y = np.full(ev.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, c["Z"], v)
            Jv[:, col] = y[row0:row0 + K * n].reshape(K, n)
            w = np.zeros(ev.n_constraints)
            w[row0:row0 + K * n] = Lam[1:, col].reshape(-1)
            y = np.full(ev.n_variables, np.nan); ev.eval_constraint_jacobian_transpose_product(y, c["Z"], w)
            JTw[:, col] = y[:N * z].reshape(N, z)[1:, x_off:x_off + n]
        errs["J v"] = rel_err(Jv, c["B"][1:])
        errs["J' w"] = rel_err(JTw, c["B"][1:])
        print(name, "K", K, errs, "bar", bar(K), "max |y|", float(np.max(np.abs(c["ref"][0]))), float(np.max(np.abs(c["ref"][1]))))
        for what, e in errs.items():
            assert e <= bar(K), (name, what, e)   # (NaN, a missing writer, fails the comparison)
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------------- tree shapes
@functools.lru_cache(maxsize=None)
def tree_case(K):
    p = scaled_case(K + 1, 12, 2)[0]
    E = propagators(p.integrators[0], p.Z0, p.N, p.z, p.dt_idx)
    B = rhs(K + 1, 2, 12, seed=K)
    ref = (recurrence(E, B, False), recurrence(E, B, True))
    for a in (E, B) + ref:
        a.setflags(write=False)
    return p, B, ref


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 9, 37, 64, 65])
def test_tree_shapes(K):
    """no level; one level; an identity leaf; the root delivers the last knot (the loader the adjoint's); mixed; dead items in several
    levels; 2^L and 2^L + 1"""
    p, B, ref = tree_case(K)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        for adjoint in (False, True):
            A = ev.dynamics_solve(p.Z0, B, adjoint=adjoint)
            err = rel_err(A, ref[adjoint])
            print("tree K=%d" % K, "adjoint" if adjoint else "forward", "rel_err", err, "bar", bar(K))
            assert err <= bar(K), (K, adjoint, err)
            F = ev.dynamics_solve(p.Z0, B, adjoint=adjoint, all_knots=False)
            assert F.shape == (2, 12) and np.array_equal(F, A[0 if adjoint else -1]), "FINAL is that block of ALL, bit for bit"
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------- adjointness and bits
@pytest.fixture(scope="module")
def ev40():
    ev = dto_amd.Evaluator(to_engine(scaled_case(6, 40, 40)[0]))
    yield ev
    ev.close()


@pytest.fixture(scope="module")
def ev70():
    ev = dto_amd.Evaluator(to_engine(scaled_case(12, 70, 3)[0]))
    yield ev
    ev.close()


def test_the_two_solves_are_adjoint_to_each_other(ev40):
    p = scaled_case(6, 40, 40)[0]
    B, Bp = rhs(6, 3, 40, seed=1), rhs(6, 3, 40, seed=2)
    Y = ev40.dynamics_solve(p.Z0, B)
    Lam = ev40.dynamics_solve(p.Z0, Bp, adjoint=True)
    for col in range(3):
        a, b = float(np.vdot(Bp[:, col], Y[:, col])), float(np.vdot(Lam[:, col], B[:, col]))
        tol = 1e-10 * (abs(a) + np.linalg.norm(B[:, col]) * np.linalg.norm(Bp[:, col]))
        print("<B', Y>", a, "<Lam, B>", b, "difference", abs(a - b), "tolerance", tol)
        assert abs(a - b) <= tol


@pytest.mark.parametrize("n", [40, 70])
def test_a_start_state_alone_gives_the_rollouts_bits(ev40, ev70, n):
    ev, (p, X0, _) = (ev40, scaled_case(6, 40, 40)) if n == 40 else (ev70, scaled_case(12, 70, 3))
    for n_cols in (1, 3):
        B = np.zeros((p.N, n_cols, n))
        B[0] = X0[:n_cols]
        assert np.array_equal(ev.dynamics_solve(p.Z0, B), ev.rollout(p.Z0, X0=X0[:n_cols])), n_cols
        assert np.array_equal(ev.dynamics_solve(p.Z0, B, all_knots=False), ev.rollout(p.Z0, X0=X0[:n_cols], all_knots=False)), n_cols


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
def test_a_column_has_the_same_bits_alone_and_among_others(ev70, adjoint):
    """17 and 40 columns run the 16-column tile, 70 the 64-column tile: the same k order, so the same bits"""
    p = scaled_case(12, 70, 3)[0]
    B = rhs(12, 70, 70, seed=5)
    alone = {c: ev70.dynamics_solve(p.Z0, B[:, c:c + 1], adjoint=adjoint)[:, 0] for c in (0, 16, 39, 69)}
    assert not np.isnan(alone[0]).any()
    for n_cols in (17, 40, 70):
        among = ev70.dynamics_solve(p.Z0, B[:, :n_cols], adjoint=adjoint)
        for c, a in alone.items():
            if c < n_cols:
                assert np.array_equal(among[:, c], a), (n_cols, c)


@pytest.mark.parametrize("where", WHERE)
def test_repeated_calls_and_both_pointer_families_are_bit_identical(places, where):
    import torch
    ev, p, Z, q, X0 = places(where)
    n, N = X0.shape[1], p.N
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    dZ = torch.from_numpy(np.array(Z)).to(dev)
    for n_cols, adjoint, all_knots in ((17, False, True), (17, True, True), (3, False, False), (3, True, False), (40, True, True)):
        n_cols = min(n_cols, n)
        B = rhs(N, n_cols, n, seed=n_cols)
        a = ev.dynamics_solve(Z, B, integrator=q, adjoint=adjoint, all_knots=all_knots)
        b = ev.dynamics_solve(Z, B, integrator=q, adjoint=adjoint, all_knots=all_knots)
        assert np.array_equal(a, b) and not np.isnan(a).any()
        if not all_knots:     # FINAL is that block of ALL, bit for bit
            assert np.array_equal(a, ev.dynamics_solve(Z, B, integrator=q, adjoint=adjoint)[0 if adjoint else -1])
        dB = torch.from_numpy(B).to(dev)
        dY = torch.full(a.shape, float("nan"), dtype=torch.float64, device=dev)
        ev.dynamics_solve_dev(dZ.data_ptr(), dB.data_ptr(), n_cols, dY.data_ptr(), integrator=q, adjoint=adjoint, all_knots=all_knots, stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(dY.cpu().numpy(), a), (n_cols, adjoint, all_knots)


@pytest.mark.parametrize("where", WHERE)
def test_a_reused_tree_gives_the_bits_of_a_rebuilt_one(places, where):
    ev, p, Z, q, X0 = places(where)
    n = X0.shape[1]
    B = rhs(p.N, 3, n, seed=8)
    Z2 = np.array(Z)
    Z2[p.dt_idx] *= 1.5
    ev.profile_enable(True)
    try:
        rebuilt, reused = {}, {}
        for adjoint in (False, True):
            ev.dynamics_solve(Z2, B, integrator=q, adjoint=adjoint)
            ev.profile_reset()
            rebuilt[adjoint] = ev.dynamics_solve(Z, B, integrator=q, adjoint=adjoint)          # Z -> Z' -> Z: a rebuild
            assert ev.profile_get("dynsolve_tree")[1] > 0
            ev.profile_reset()
            reused[adjoint] = ev.dynamics_solve(Z, B, integrator=q, adjoint=adjoint)
            assert ev.profile_get("dynsolve_tree")[1] == 0
            assert np.array_equal(rebuilt[adjoint], reused[adjoint])
        assert not np.array_equal(rebuilt[False], ev.dynamics_solve(Z2, B, integrator=q))     # (the other point is another point)
    finally:
        ev.profile_enable(False)


# ------------------------------------------------------------------------------------------------------------ the cache
def test_the_tree_is_kept_per_point():
    p, X0, _ = scaled_case(12, 70, 3)
    B = rhs(12, 3, 70, seed=3)
    ev = dto_amd.Evaluator(to_engine(p))

    def counts(Z, adjoint):
        ev.profile_reset()
        ev.dynamics_solve(Z, B, adjoint=adjoint)
        every, tree, scan, whole = (ev.profile_get(name) for name in ("all", "dynsolve_tree", "dynsolve_scan", "dynsolve"))
        assert scan[1] > 0 and whole[1] == tree[1] + scan[1] and whole[2] == tree[2] + scan[2]
        assert ev.profile_get("rollout")[1] == 0
        return every[1], tree[1]

    try:
        ev.profile_enable(True)
        first = counts(p.Z0, False)
        assert first[0] > 0 and first[1] == 1 + 4          # the gather and L = 4 levels of products
        assert counts(p.Z0, False) == (0, 0)                # the same point
        assert counts(p.Z0, True) == (0, 0)                 # ... in the other direction too
        Z = np.array(p.Z0)
        Z[p.dt_idx] = np.nextafter(Z[p.dt_idx], np.inf)     # one bit of Z
        a = counts(Z, True)
        assert a[0] > 0 and a[1] > 0
        assert counts(Z, False) == (0, 0)
        ev.set_option("overlap_sweep", 0)
        a = counts(Z, False)
        assert a[0] > 0 and a[1] > 0
        assert counts(Z, True) == (0, 0)
        ev.rollout(Z, X0=X0)                                # overwrites the tree
        a = counts(Z, True)
        assert a[0] > 0 and a[1] > 0
        assert counts(Z, True) == (0, 0)
        ev.profile_enable(False)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("kind", ["bilinear", "k_tdb"])
def test_rollout_gradient_against_central_differences(kind):
    """phi = 1/2 |x_N - goal|^2 of the rolled-out final state; <rollout_gradient, d> against (phi(Z + h d) - phi(Z - h d)) / 2h,
    h = 1e-5, on five directions in the non-state components, to relative 1e-6 (the reference's own finite-difference bar)."""
    p = scaled_case(9, 12, 2)[0] if kind == "bilinear" else O.make_tdb_problem(N=6, n=4, m=2, substeps=16)
    it = p.integrators[0]
    n, N, z = it.x_dim, p.N, p.z
    rng = np.random.default_rng(17)
    goal = rng.standard_normal(n)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        def phi(Z):
            return 0.5 * float(np.sum((ev.rollout(Z, all_knots=False)[0] - goal) ** 2))

        Z = np.array(p.Z0)
        C = np.zeros((N, n))
        C[-1] = ev.rollout(Z, all_knots=False)[0] - goal
        g = ev.rollout_gradient(Z, C)
        assert g.shape == (ev.n_variables,) and not np.isnan(g).any()
        assert np.all(g[:N * z].reshape(N, z)[:, it.x_off:it.x_off + n] == 0.0)
        h = 1e-5
        for trial in range(5):
            d = np.zeros(ev.n_variables)
            dk = d[:N * z].reshape(N, z)
            dk[:] = rng.standard_normal((N, z))
            dk[:, it.x_off:it.x_off + n] = 0.0
            fd = (phi(Z + h * d) - phi(Z - h * d)) / (2.0 * h)
            an = float(g @ d)
            rel = abs(an - fd) / max(abs(an), abs(fd))
            print(kind, "direction", trial, "analytic", an, "central difference", fd, "relative", rel)
            assert rel <= 1e-6, (kind, trial, rel)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_reason_and_leave_the_handle_usable(ev40):
    p = scaled_case(6, 40, 40)[0]
    lib, dp = dto_amd.load_library(), dto_amd.capi.c_double_p
    B = rhs(6, 3, 40, seed=4)
    with pytest.raises(dto_amd.EngineError, match="n_cols = 0"):
        ev40.dynamics_solve(p.Z0, np.empty((6, 0, 40)))
    with pytest.raises(dto_amd.EngineError, match="n_cols = 41"):
        ev40.dynamics_solve(p.Z0, np.ones((6, 41, 40)))
    Z, b, out = np.array(p.Z0), np.array(B[:, :1]), np.full((6, 1, 40), np.nan)
    args = lambda direction, bp, mode: (ev40.handle, 0, Z.ctypes.data_as(dp), direction, bp, 1, mode, out.ctypes.data_as(dp))
    assert lib.dto_dynamics_solve(*args(0, b.ctypes.data_as(dp), 2)) != 0
    assert "mode" in lib.dto_last_error(ev40.handle).decode() and np.isnan(out).all()
    for direction in (-1, 2):
        assert lib.dto_dynamics_solve(*args(direction, b.ctypes.data_as(dp), 0)) != 0
        assert "direction" in lib.dto_last_error(ev40.handle).decode() and np.isnan(out).all()
    assert lib.dto_dynamics_solve(*args(1, None, 0)) != 0
    assert "B = NULL" in lib.dto_last_error(ev40.handle).decode() and np.isnan(out).all()
    for bad in (-1, 2):   # the handle has two integrators
        with pytest.raises(dto_amd.EngineError, match="out of range"):
            ev40.dynamics_solve(p.Z0, np.ones((6, 1, 1)), integrator=bad)
    with pytest.raises(dto_amd.EngineError, match="DerivativeIntegrator"):
        ev40.dynamics_solve(p.Z0, np.ones((6, 1, 2)), integrator=1)
    E = propagators(p.integrators[0], p.Z0, p.N, p.z, p.dt_idx)
    assert rel_err(ev40.dynamics_solve(p.Z0, B, adjoint=True), recurrence(E, B, True)) <= bar(5)   # the handle stays usable


def test_external_integrators_and_sharded_handles_are_refused():
    p = O.make_external_integrator_problem()
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        ext = [i for i, it in enumerate(p.integrators) if it.kind == "external"][0]
        with pytest.raises(dto_amd.EngineError, match="evaluated on the host"):
            ev.dynamics_solve(p.Z0, np.ones((p.N, 1, p.integrators[ext].x_dim)), integrator=ext)
        g = np.full(ev.n_constraints, np.nan); ev.eval_constraint(g, p.Z0)
        assert not np.isnan(g).any()
    finally:
        ev.close()
    p = scaled_case(6, 40, 40)[0]
    ev = dto_amd.Evaluator(to_engine(p), k_lo=1, k_hi=3)
    try:
        with pytest.raises(dto_amd.EngineError, match="unsharded"):
            ev.dynamics_solve(p.Z0, np.ones((6, 1, 40)))
        g = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(g, p.Z0)
        assert not np.isnan(g).any()
    finally:
        ev.close()

