"""GPU: the whole-dynamics solves (dto_dynamics_solve_all / dto_dynamics_solve_all_dev, csrc/dto_elim.hip) -- solves with the Jacobian
block MM of ALL integrators' rows and ALL their state columns.

Reference, independent of the engine: numpy.linalg.solve on MM assembled from the ORACLE's Jacobian (elim_cases.case).  Bar:
rel_err <= bar(K) x levels with bar(K) = helpers.TOL max(1, K / 16), the single-integrator solves' bar (tests/test_gpu_rollout.py) --
each level adds one block solve held to that bar and one contraction with Jacobian entries held to TOL.  The cases have skew
generators or few knots, cond(MM) below a few hundred (the unskewed scaling problem, cond 6e5, is no test of the kernels).  The same
results are checked against the engine's own Jacobian, its J w, and each other (adjointness).  Outputs are pre-filled with NaN so that
a missing writer shows.  The largest errors seen are in DESIGN 4.26."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from elim_cases import CASES, REFUSED_LAYOUTS, RawDerivativeHandle, assemble, case, engine_jacobian_dense
from helpers import rel_err, to_engine
from test_gpu_rollout import bar

pytestmark = pytest.mark.gpu


def flat(A):
    """(N, n_cols, D) -> (N D, n_cols): MM's index order"""
    N, nc, D = A.shape
    return A.transpose(0, 2, 1).reshape(N * D, nc)


def evaluator(c):
    return dto_amd.Evaluator(c["pe"], **c["kw"])


def device_arrays(*arrays):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays], torch.cuda.current_stream(dev).cuda_stream


# ----------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", CASES)
def test_values_against_the_dense_solve_and_the_engines_own_jacobian(name):
    c = case(name)
    p, Z, B = c["p"], c["Z"], c["B"]
    N, K, D, levels = p.N, p.N - 1, c["D"], c["plan"]["n_levels"]
    limit = bar(K) * levels
    ev = evaluator(c)
    try:
        assert ev.dynamics_layout() [:2] == (D, levels)
        assert list(ev.dynamics_layout()[2]) == c["plan"]["pre"] and list(ev.dynamics_layout()[3]) == c["plan"]["level"]
        Y = ev.dynamics_solve_all(Z, B)
        Lam = ev.dynamics_solve_all(Z, B, adjoint=True)
        assert Y.shape == Lam.shape == B.shape
        errs = dict(forward=rel_err(Y, c["ref"][0]), adjoint=rel_err(Lam, c["ref"][1]))
        # MM from the engine's own Jacobian values: MM Y = B, MM' Lam = B
        Me = assemble(engine_jacobian_dense(ev, Z), p)
        errs["MM Y"] = rel_err(Me @ flat(Y), flat(B))
        errs["MM' Lam"] = rel_err(Me.T @ flat(Lam), flat(B))
        # J w with Y in the state columns returns B_{k+1} in every integrator's rows
        Jv = np.empty((K, 3, D))
        for col in range(3):
            v = np.zeros(ev.n_variables)
            vk = v[:N * p.z].reshape(N, p.z)
            for i, it in enumerate(p.integrators):
                vk[:, it.x_off:it.x_off + it.x_dim] = Y[:, col, c["plan"]["pre"][i]:c["plan"]["pre"][i] + it.x_dim]
            y = np.full(ev.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, Z, v)
            for i, it in enumerate(p.integrators):
                row0 = K * c["plan"]["pre"][i]
                Jv[:, col, c["plan"]["pre"][i]:c["plan"]["pre"][i] + it.x_dim] = y[row0:row0 + K * it.x_dim].reshape(K, it.x_dim)
        errs["J w"] = rel_err(Jv, B[1:])
        print(name, "K", K, "levels", levels, errs, "bar", limit, "cond", float(np.linalg.cond(c["M"])), "max |y|",
              float(np.max(np.abs(c["ref"][0]))), float(np.max(np.abs(c["ref"][1]))))
        for what, e in errs.items():
            assert e <= limit, (name, what, e)   # (NaN, a missing writer, fails the comparison)
    finally:
        ev.close()


def test_the_two_solves_are_adjoint_to_each_other():
    c = case("three_level_40x6")
    Bp = np.random.default_rng(2).standard_normal(c["B"].shape)
    ev = evaluator(c)
    try:
        Y = ev.dynamics_solve_all(c["Z"], c["B"])
        Lam = ev.dynamics_solve_all(c["Z"], Bp, adjoint=True)
        for col in range(3):
            a, b = float(np.vdot(Bp[:, col], Y[:, col])), float(np.vdot(Lam[:, col], c["B"][:, col]))
            tol = 1e-10 * (abs(a) + np.linalg.norm(c["B"][:, col]) * np.linalg.norm(Bp[:, col]))
            print("<C, Y(B)>", a, "<Lam(C), B>", b, "difference", abs(a - b), "tolerance", tol)
            assert abs(a - b) <= tol
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------------- bits
def loop(B, adjoint):
    Y = np.empty_like(B)
    if adjoint:
        Y[-1] = B[-1]
        for k in range(B.shape[0] - 2, -1, -1):
            Y[k] = Y[k + 1] + B[k]
    else:
        Y[0] = B[0]
        for k in range(B.shape[0] - 1):
            Y[k + 1] = Y[k] + B[k + 1]
    return Y


def test_a_level_0_derivative_block_is_the_numpy_loop_bit_for_bit():
    c = case("scaled_12x9")      # [bilinear, derivative]: the derivative integrator is level 0
    ev = evaluator(c)
    try:
        sl = slice(c["plan"]["pre"][1], c["D"])
        assert np.array_equal(ev.dynamics_solve_all(c["Z"], c["B"])[:, :, sl], loop(c["B"][:, :, sl], False))
    finally:
        ev.close()
    h = RawDerivativeHandle([(0, 3, 3)], 7, N=37, device=0)   # derivative integrators only: both directions, up to 64 columns
    try:
        for n_cols in (1, 5, 64):
            B = np.random.default_rng(n_cols).standard_normal((37, n_cols, 3))
            for adjoint in (False, True):
                Y, text = h.solve(B, adjoint)
                assert text is None and np.array_equal(Y, loop(B, adjoint)), (n_cols, adjoint)
        Y, text = h.solve(np.ones((37, 65, 3)))
        assert Y is None and "n_cols = 65, allowed 1 .. 64" in text
    finally:
        h.close()


@pytest.fixture(scope="module")
def ev3():
    ev = evaluator(case("three_level_40x6"))
    yield ev
    ev.close()


def test_repeated_calls_and_both_pointer_families_are_bit_identical(ev3):
    import torch
    c = case("three_level_40x6")
    (dZ,), st = device_arrays(c["Z"])
    for n_cols, adjoint in ((1, False), (3, True), (17, False), (40, True)):
        B = np.random.default_rng(n_cols).standard_normal((c["p"].N, n_cols, c["D"]))
        a = ev3.dynamics_solve_all(c["Z"], B, adjoint=adjoint)
        b = ev3.dynamics_solve_all(c["Z"], B, adjoint=adjoint)
        assert np.array_equal(a, b) and not np.isnan(a).any()
        (dB,), _ = device_arrays(B)
        dY = torch.full(a.shape, float("nan"), dtype=torch.float64, device=dB.device)
        ev3.dynamics_solve_all_dev(dZ.data_ptr(), dB.data_ptr(), n_cols, dY.data_ptr(), adjoint=adjoint, stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(dY.cpu().numpy(), a), (n_cols, adjoint)


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
def test_a_column_has_the_same_bits_alone_and_among_others(ev3, adjoint):
    """17 columns run the block solves' 16-column tile twice, 40 three times; the contractions are a thread per entry"""
    c = case("three_level_40x6")
    B = np.random.default_rng(5).standard_normal((c["p"].N, 40, c["D"]))
    alone = {col: ev3.dynamics_solve_all(c["Z"], B[:, col:col + 1], adjoint=adjoint)[:, 0] for col in (0, 16, 39)}
    assert not np.isnan(alone[0]).any()
    for n_cols in (17, 40):
        among = ev3.dynamics_solve_all(c["Z"], B[:, :n_cols], adjoint=adjoint)
        for col, a in alone.items():
            if col < n_cols:
                assert np.array_equal(among[:, col], a), (n_cols, col)


# ------------------------------------------------------------------------------------------------------------ the cache
def launches(ev, *names):
    return tuple(ev.profile_get(n)[1] for n in names)


@pytest.mark.parametrize("name", ["scaled_40x6", "multi_ket_between", "scaled_70x12"], ids=["one_ket", "two_kets", "general_path"])
def test_one_jacobian_per_new_point_and_none_at_the_cached_point(name):
    import torch
    c = case(name)
    Z, B, n_int = c["Z"], c["B"], len(c["p"].integrators)
    pairs = sum(len(d) for d in c["plan"]["deps"])
    trees = sum(1 for it in c["p"].integrators if it.kind != "derivative")
    Z2 = np.array(Z)
    Z2[c["p"].dt_idx] *= 1.5
    ev = evaluator(c)
    try:
        (dZ,), st = device_arrays(Z)
        dvals = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dZ.device)
        ev.profile_enable(True)
        ev.eval_jacobian_dev(dZ.data_ptr(), dvals.data_ptr(), stream=st)
        torch.cuda.synchronize()
        jac = launches(ev, "bgemm", "chain64")
        assert sum(jac) > 0
        ev.profile_reset()
        first = ev.dynamics_solve_all(Z, B)                                    # a new point
        assert launches(ev, "bgemm", "chain64") == jac, "the chain runs once, however many integrators there are"
        L = int(np.ceil(np.log2(max(c["p"].N - 1, 1))))
        assert launches(ev, "dynsolve_tree") == (trees * (1 + L),) and launches(ev, "dynsolve_couple") == (pairs + n_int,)
        assert launches(ev, "dynsolve_deriv") == (n_int - trees,) and launches(ev, "rollout") == (0,)
        ev.profile_reset()
        again = ev.dynamics_solve_all(Z, B)                                    # the cached point
        lam = ev.dynamics_solve_all(Z, B, adjoint=True)                        # ... in the other direction too
        assert launches(ev, "all", "bgemm", "chain64", "dynsolve_tree") == (0, 0, 0, 0)
        assert launches(ev, "dynsolve_couple") == (2 * n_int,), "the contractions alone: no gather"
        assert np.array_equal(first, again)
        ev.rollout(Z2)                                                         # another point, another call's workspace
        ev.dynamics_solve(Z2, np.ones((c["p"].N, 1, c["p"].integrators[0].x_dim)))
        ev.profile_reset()
        assert np.array_equal(ev.dynamics_solve_all(Z, B, adjoint=True), lam)
        assert launches(ev, "all", "dynsolve_tree") == (0, 0), "dto_rollout and dto_dynamics_solve do not disturb the cached point"
        ev.set_option("overlap_sweep", 0)
        ev.profile_reset()
        rebuilt = ev.dynamics_solve_all(Z, B)
        assert launches(ev, "dynsolve_tree") == (trees * (1 + L),) and launches(ev, "all")[0] > 0, "dto_set_option makes it rebuild"
        assert np.array_equal(rebuilt, first), "rebuilt and cached give the same bits"
        ev.profile_reset()
        other = ev.dynamics_solve_all(Z2, B)                                   # one more point, and back
        assert launches(ev, "dynsolve_tree")[0] > 0 and not np.array_equal(other, first)
        assert np.array_equal(ev.dynamics_solve_all(Z, B), first)
        ev.profile_enable(False)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_reason_and_leave_the_handle_usable(ev3):
    c = case("three_level_40x6")
    N, D = c["p"].N, c["D"]
    lib, dp = dto_amd.load_library(), dto_amd.capi.c_double_p
    with pytest.raises(dto_amd.EngineError, match="n_cols = 0"):
        ev3.dynamics_solve_all(c["Z"], np.empty((N, 0, D)))
    with pytest.raises(dto_amd.EngineError, match="n_cols = 41, allowed 1 .. 40"):
        ev3.dynamics_solve_all(c["Z"], np.ones((N, 41, D)))
    Z, b, out = np.array(c["Z"]), np.array(c["B"][:, :1]), np.full((N, 1, D), np.nan)
    for direction in (-1, 2):
        assert lib.dto_dynamics_solve_all(ev3.handle, Z.ctypes.data_as(dp), direction, b.ctypes.data_as(dp), 1, out.ctypes.data_as(dp)) != 0
        assert "direction" in lib.dto_last_error(ev3.handle).decode() and np.isnan(out).all()
    assert lib.dto_dynamics_solve_all(ev3.handle, Z.ctypes.data_as(dp), 1, None, 1, out.ctypes.data_as(dp)) != 0
    assert "B = NULL" in lib.dto_last_error(ev3.handle).decode() and np.isnan(out).all()
    assert lib.dto_dynamics_solve_all_dev(ev3.handle, None, 0, None, 1, None, None) != 0
    assert "B = NULL" in lib.dto_last_error(ev3.handle).decode()
    assert rel_err(ev3.dynamics_solve_all(c["Z"], c["B"], adjoint=True), c["ref"][1]) <= 3 * bar(N - 1)   # the handle stays usable


@pytest.mark.parametrize("name", list(REFUSED_LAYOUTS))
def test_the_plan_refusals_on_a_device_handle(name):
    integs, z, text = REFUSED_LAYOUTS[name]
    h = RawDerivativeHandle(integs, z, device=0)
    try:
        Y, said = h.solve(np.ones((h.N, 1, h.D)))
        assert Y is None and text in said and said.startswith("dto_dynamics_solve_all")
        assert text in h.layout()
    finally:
        h.close()


def test_external_integrators_and_sharded_handles_are_refused():
    p = O.make_external_integrator_problem()
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        D = sum(it.x_dim for it in p.integrators)
        with pytest.raises(dto_amd.EngineError, match="evaluated on the host"):
            ev.dynamics_solve_all(p.Z0, np.ones((p.N, 1, D)))
        g = np.full(ev.n_constraints, np.nan); ev.eval_constraint(g, p.Z0)
        assert not np.isnan(g).any()
    finally:
        ev.close()
    c = case("scaled_40x6")
    ev = dto_amd.Evaluator(c["pe"], k_lo=1, k_hi=3)
    try:
        with pytest.raises(dto_amd.EngineError, match="unsharded"):
            ev.dynamics_solve_all(c["Z"], c["B"])
        g = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(g, c["Z"])
        assert not np.isnan(g).any()
    finally:
        ev.close()


# ----------------------------------------------------------------------------------------------------- reduced gradient
@functools.lru_cache(maxsize=None)
def gradient_problem(kind):
    """12 x 9 bilinear and k_tdb at 4 x 6, each with its derivative integrator; besides the regularizer on u a terminal
    ||x_N - goal||^2, so that f sees the states of both levels"""
    p = O.make_scaled_problem(9, 12, 2, seed=321, skew=True) if kind == "bilinear" else \
        O.make_tdb_problem(N=6, n=4, m=2, substeps=16, with_derivative=True)
    n = p.integrators[0].x_dim
    p.objectives.append(O.KnotSqDistObjective(list(range(n)), [p.N], [1.0], np.random.default_rng(3).standard_normal((1, n))))
    return p


@pytest.mark.parametrize("kind", ["bilinear", "k_tdb"])
def test_reduced_gradient_against_central_differences(kind):
    """<reduced_gradient(Z*), d> against (f(feasible(Z* + h d)) - f(feasible(Z* - h d))) / 2h at Z* = feasible_trajectory(Z0): h = 1e-5,
    five directions in everything the states of knots 2 .. N are a function of (controls, timesteps, times, the states of knot 1), to
    relative 1e-6 -- step, count and bar of the rollout_gradient test."""
    p = gradient_problem(kind)
    N, z = p.N, p.z
    rng = np.random.default_rng(17)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        def f(Z):
            return ev.eval_objective(ev.feasible_trajectory(Z))

        Zs = ev.feasible_trajectory(p.Z0)
        g = np.full(ev.n_constraints, np.nan); ev.eval_constraint(g, Zs)
        assert np.max(np.abs(g[:ev.n_dynamics_constraints])) <= 1e-9, "the feasible trajectory satisfies the dynamics"
        assert np.array_equal(ev.feasible_trajectory(Zs).reshape(-1)[:z], Zs[:z])
        r = ev.reduced_gradient(Zs)
        assert r.shape == (ev.n_variables,) and not np.isnan(r).any()
        rk = r[:N * z].reshape(N, z)
        for it in p.integrators:
            assert np.all(rk[1:, it.x_off:it.x_off + it.x_dim] == 0.0)
        h = 1e-5
        for trial in range(5):
            d = np.zeros(ev.n_variables)
            dk = d[:N * z].reshape(N, z)
            dk[:] = rng.standard_normal((N, z))
            for it in p.integrators:
                dk[1:, it.x_off:it.x_off + it.x_dim] = 0.0
            fd = (f(Zs + h * d) - f(Zs - h * d)) / (2.0 * h)
            an = float(r @ d)
            rel = abs(an - fd) / max(abs(an), abs(fd))
            print(kind, "direction", trial, "analytic", an, "central difference", fd, "relative", rel)
            assert rel <= 1e-6, (kind, trial, rel)
    finally:
        ev.close()
