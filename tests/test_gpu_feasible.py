"""GPU: the device feasible-trajectory rollout and the reduced merit value (dto_feasible_trajectory / dto_feasible_merit and their _dev
forms, csrc/dto_feasible.hip, csrc/dto_feasible_plan.h).

Three references.  The YARDSTICK, Evaluator.feasible_trajectory: the host loop over levels and integrators with one dto_rollout per
propagating integrator -- the engine call must return its bits.  The ORACLE, reduced_cases.oracle_feasible: Newton on the dynamics rows
with the oracle's Jacobian, held to 1e-10 x levels x max(1, K / 16) (the whole-dynamics solves' bar times the rollout's).  The merit
value's stated summation order written in NumPy, bit for bit.  Outputs are pre-filled with NaN, so a missing writer shows."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import reduced_cases as R
from elim_cases import RawDerivativeHandle
from helpers import rel_err, to_engine
from test_gpu_rollout import bar

pytestmark = pytest.mark.gpu

# small path; one-launch chain; general path, padded to 128; three levels; two kets on one level; both spline orders; structured path
BIT_CASES = ["scaled_12x9", "scaled_40x6", "scaled_70x5", "three_level_40x6", "multi_ket_between", "tdb_order0", "tdb_order1",
             "structured_16x4"]
MERIT_CASES = ["scaled_12x9+con", "scaled_12x70+con"]     # 7 constraint rows (fewer than 64); 68: lanes holding two rows and one


def device_arrays(*arrays):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays], torch.cuda.current_stream(dev).cuda_stream


def launches(ev, *names):
    return tuple(ev.profile_get(n)[1] for n in names)


@functools.lru_cache(maxsize=None)
def case(name):
    if name != "scaled_12x70+con":
        return R.case(name)
    p = O.make_scaled_problem(70, 12, 2, skew=True, with_constraint=True)
    n_dyn = sum(it.x_dim for it in p.integrators) * (p.N - 1)
    n_cons = n_dyn + sum(c.g_dim * len(c.times1) for c in p.constraints)
    mu = np.zeros(n_cons)
    mu[n_dyn:] = np.random.default_rng(12).standard_normal(n_cons - n_dyn)
    Z = np.ascontiguousarray(p.Z0, dtype=np.float64)
    Z.setflags(write=False); mu.setflags(write=False)
    return dict(p=p, pe=to_engine(p), kw={}, Z=Z, mu=mu, levels=2, n_cons=n_cons, n_dyn=n_dyn)


def evaluator(c, **kw):
    return dto_amd.Evaluator(c["pe"], **dict(c["kw"], **kw))


@functools.lru_cache(maxsize=None)
def trajectories(name):
    """the engine's three forms on one handle, the yardstick on a handle of its own: computed once per case"""
    import torch
    c = case(name)
    Z = c["Z"]
    ev = evaluator(c)
    try:
        host = ev.feasible_trajectory_engine(Z)
        (dZ,), st = device_arrays(Z)
        dZf = torch.full_like(dZ, float("nan"))
        ev.feasible_trajectory_dev(dZ.data_ptr(), dZf.data_ptr(), stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(dZ.cpu().numpy(), Z), "out of place: Z is not written"
        out_of_place = dZf.cpu().numpy()
        ev.feasible_trajectory_dev(dZ.data_ptr(), dZ.data_ptr(), stream=st)
        torch.cuda.synchronize()
        in_place = dZ.cpu().numpy()
        again = ev.feasible_trajectory_engine(Z)
    finally:
        ev.close()
    ev = evaluator(c)
    try:
        yardstick = ev.feasible_trajectory(Z)
    finally:
        ev.close()
    return dict(host=host, out_of_place=out_of_place, in_place=in_place, again=again, yardstick=yardstick)


# ------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("name", BIT_CASES)
def test_bit_identity_with_the_host_composition(name):
    t = trajectories(name)
    assert not np.isnan(t["yardstick"]).any()
    for form in ("host", "out_of_place", "in_place", "again"):
        assert not np.isnan(t[form]).any(), form
        assert np.array_equal(t[form], t["yardstick"]), form


@pytest.mark.parametrize("N", [4, 150])
def test_a_lone_derivative_integrator_is_the_numpy_recurrence_bit_for_bit(N):
    """70 components: two workgroups of the recurrence kernel (64 and 6 components), no propagator, no Jacobian.  N = 150: the first
    workgroup walks its 149 intervals in chunks of 64, 64 and 21 knots (4096 / 64 per chunk), the second in one chunk"""
    d = 70
    h = RawDerivativeHandle([(0, d, d)], 2 * d + 1, N=N, device=0, seed=5)
    try:
        dp = dto_amd.capi.c_double_p
        Zk = np.array(h.Z).reshape(N, h.z)
        for k in range(N - 1):
            Zk[k + 1, :d] = Zk[k, :d] + Zk[k, h.z - 1] * Zk[k, d:2 * d]
        Zf = np.full(h.Z.size, np.nan)
        assert h.lib.dto_profile_enable(h.h, 1) == 0
        assert h.lib.dto_feasible_trajectory(h.h, h.Z.ctypes.data_as(dp), Zf.ctypes.data_as(dp)) == 0, h.lib.dto_last_error(h.h).decode()
        assert np.array_equal(Zf, Zk.reshape(-1))
        import ctypes as C
        ms, n, by = C.c_double(), C.c_int64(), C.c_double()
        for name, want in (("feasible", 1), ("all", 0), ("rollout", 0)):
            assert h.lib.dto_profile_get(h.h, name.encode(), C.byref(ms), C.byref(n), C.byref(by)) == 0
            assert n.value == want, (name, n.value)
    finally:
        h.close()


# ----------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", BIT_CASES)
def test_values_against_the_oracle(name):
    c, t = case(name), trajectories(name)
    p = c["p"]
    ref = R.oracle_feasible(p, c["Z"])
    err, b = rel_err(t["host"], ref), c["levels"] * bar(p.N - 1)
    print(name, "feasible trajectory against the oracle: error", err, "bar", b)
    assert err <= b
    S, C_, _, _ = R.index_sets(p)
    assert np.array_equal(t["host"][C_], c["Z"][C_]), "controls, timesteps, times, the states of knot 1 and globals are copies"
    assert not np.array_equal(t["host"][S], c["Z"][S])


# ------------------------------------------------------------------------------------------------------------------ merit
def merit_in_numpy(sigma, f, mu, g, n_dyn):
    """the header's order: lane l adds mu_r g_r over r = n_dyn + l, n_dyn + l + 64, ..; the halving tree; sigma * f + t"""
    if mu is None:
        return sigma * f
    p = np.zeros(64)
    rows = np.arange(n_dyn, g.size)
    for s in range(0, rows.size, 64):
        idx = rows[s:s + 64]
        p[:idx.size] = p[:idx.size] + mu[idx] * g[idx]
    off = 32
    while off >= 1:
        p[:off] = p[:off] + p[off:2 * off]
        off //= 2
    return sigma * f + p[0]


@functools.lru_cache(maxsize=None)
def merits(name):
    import torch
    c = case(name)
    Z, n_dyn = c["Z"], c["n_dyn"]
    mu = np.array(c["mu"])
    mu[:n_dyn] = np.nan     # the dynamics-row entries of mu are never read
    ev = evaluator(c)
    try:
        phi, Zf, g = ev.feasible_merit(Z, R.SIGMA, mu, trajectory=True, constraints=True)
        phi_again = ev.feasible_merit(Z, R.SIGMA, mu)
        phi_none, g_none = ev.feasible_merit(Z, R.SIGMA, None, constraints=True)
        f = ev.eval_objective(Zf)
        g_cb = np.full(ev.n_constraints, np.nan); ev.eval_constraint(g_cb, Zf)
        (dZ, dmu), st = device_arrays(Z, mu)
        dphi = torch.full((1,), float("nan"), dtype=torch.float64, device=dZ.device)
        dZf, dg = torch.full_like(dZ, float("nan")), torch.full_like(dmu, float("nan"))
        ev.feasible_merit_dev(dZ.data_ptr(), R.SIGMA, dmu.data_ptr(), dphi.data_ptr(), dZf.data_ptr(), dg.data_ptr(), stream=st)
        torch.cuda.synchronize()
        dev = (float(dphi.cpu()[0]), dZf.cpu().numpy(), dg.cpu().numpy())
        dphi.fill_(float("nan"))
        ev.feasible_merit_dev(dZ.data_ptr(), R.SIGMA, dmu.data_ptr(), dphi.data_ptr(), stream=st)     # the engine's own Zf and g
        torch.cuda.synchronize()
        dev_bare = float(dphi.cpu()[0])
        traj = ev.feasible_trajectory_engine(Z)
    finally:
        ev.close()
    return dict(phi=phi, Zf=Zf, g=g, phi_again=phi_again, phi_none=phi_none, g_none=g_none, f=f, g_cb=g_cb, dev=dev, dev_bare=dev_bare,
                traj=traj, mu=mu)


@pytest.mark.parametrize("name", MERIT_CASES)
def test_the_merit_value_has_the_stated_bits(name):
    c, m = case(name), merits(name)
    n_dyn = c["n_dyn"]
    assert np.isfinite(m["phi"]) and not np.isnan(m["Zf"]).any() and not np.isnan(m["g"]).any()
    assert np.array_equal(m["Zf"], m["traj"]), "the merit's trajectory is dto_feasible_trajectory's"
    assert np.array_equal(m["g"], m["g_cb"]), "g is dto_eval_constraint at Zf, bit for bit"
    want = merit_in_numpy(R.SIGMA, m["f"], m["mu"], m["g_cb"], n_dyn)
    print(name, "phi", m["phi"], "in NumPy", want, "rows", m["g"].size - n_dyn, "largest defect", np.max(np.abs(m["g"][:n_dyn])))
    assert m["phi"] == want
    assert m["phi"] != R.SIGMA * m["f"], "the constraint rows take part"
    assert m["phi_none"] == R.SIGMA * m["f"] and np.array_equal(m["g_none"], m["g"]), "mu = None: sigma * f"
    assert m["phi_again"] == m["phi"], "a repeated call returns the same bits"
    assert m["dev"][0] == m["phi"] and np.array_equal(m["dev"][1], m["Zf"]) and np.array_equal(m["dev"][2], m["g"]), "both families"
    assert m["dev_bare"] == m["phi"], "Zf and g in the engine's own buffers"
    assert np.max(np.abs(m["g"][:n_dyn])) <= 1e-9, "the dynamics rows of g are the defects the rollout leaves"


@pytest.mark.parametrize("name", ["three_level_40x6", "tdb_order1", "structured_16x4"])
def test_the_defects_of_the_rollout(name):
    c = case(name)
    ev = evaluator(c)
    try:
        phi, g = ev.feasible_merit(c["Z"], 1.0, None, constraints=True)
        assert np.isfinite(phi) and not np.isnan(g).any()
        print(name, "largest defect", np.max(np.abs(g[:c["n_dyn"]])))
        assert np.max(np.abs(g[:c["n_dyn"]])) <= 1e-9
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------- central differences
@pytest.mark.parametrize("name", ["scaled_12x9+con", "tdb_order1"])
def test_the_reduced_gradient_is_the_merit_values_derivative(name):
    """(phi(Z* + h d) - phi(Z* - h d)) / 2h against <reduced_lagrangian_gradient(Z*, sigma, mu), d> at Z* = the feasible trajectory of
    Z0: h = 1e-5, three free directions, relative 1e-6 -- step, count and bar of the central-difference tests of the reduced operators"""
    c = case(name)
    p, mu = c["p"], c["mu"]
    rng = np.random.default_rng(29)
    ev = evaluator(c)
    try:
        Zs = ev.feasible_trajectory_engine(c["Z"])
        r = ev.reduced_lagrangian_gradient(Zs, R.SIGMA, mu)
        h = 1e-5
        for trial in range(3):
            d = R.free_direction(p, rng)
            fd = (ev.feasible_merit(Zs + h * d, R.SIGMA, mu) - ev.feasible_merit(Zs - h * d, R.SIGMA, mu)) / (2.0 * h)
            an = float(r @ d)
            rel = abs(an - fd) / max(abs(an), abs(fd))
            print(name, "direction", trial, "analytic", an, "central difference", fd, "relative", rel)
            assert rel <= 1e-6, (name, trial, rel)
    finally:
        ev.close()


# ----------------------------------------------------------------------------------------------------- launch accounting
@pytest.mark.parametrize("name", ["scaled_40x6", "multi_ket_between", "scaled_70x5"], ids=["one_ket", "two_kets", "general_path"])
def test_one_jacobian_per_level_with_a_propagator(name):
    import torch
    c = case(name)
    kets = sum(1 for it in c["p"].integrators if it.kind != "derivative")
    n_int = len(c["p"].integrators)
    ev = evaluator(c)
    try:
        Zs = ev.feasible_trajectory_engine(c["Z"])     # a feasible point: every Jacobian below is evaluated at exactly these bits
        (dZ,), st = device_arrays(Zs)
        dZf = torch.full_like(dZ, float("nan"))
        dvals = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dZ.device)
        ev.profile_enable(True)
        ev.eval_jacobian_dev(dZ.data_ptr(), dvals.data_ptr(), stream=st)
        torch.cuda.synchronize()
        jac, jac_all = launches(ev, "bgemm", "chain64"), launches(ev, "all")
        assert sum(jac) > 0
        ev.profile_reset()
        ev.feasible_trajectory_dev(dZ.data_ptr(), dZf.data_ptr(), stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(dZf.cpu().numpy(), Zs), "the rollout of a feasible trajectory is that trajectory"
        print(name, "feasible_trajectory_dev: bgemm, chain64", launches(ev, "bgemm", "chain64"), "of one Jacobian", jac, "feasible",
              ev.profile_get("feasible"))
        assert launches(ev, "bgemm", "chain64") == jac, "the chain runs as often as in ONE eval_jacobian_dev"
        ms, n, nbytes = ev.profile_get("feasible")
        assert n == n_int and nbytes > 0, "one launch per DERIV and ROLL step, bytes as executed"
        assert launches(ev, "all") == jac_all, "the feasible launches feed no other name"
        L = int(np.ceil(np.log2(max(c["p"].N - 1, 1))))
        assert launches(ev, "rollout_gather", "rollout_tree") == (kets, kets * L)
        ev.profile_reset()
        ev.feasible_merit(Zs, R.SIGMA, None)
        assert launches(ev, "feasible") == (n_int + 1,) and launches(ev, "bgemm", "chain64") == jac
        ev.profile_reset()
        assert np.array_equal(ev.feasible_trajectory(Zs), Zs)     # the host composition: one Jacobian per ket
        assert launches(ev, "bgemm", "chain64") == tuple(kets * j for j in jac)
        assert launches(ev, "feasible") == (0,)
        ev.profile_enable(False)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------ kept points
def test_a_merit_value_between_two_reduced_products_costs_them_nothing():
    c = case("scaled_40x6+con")
    Z, mu, v = c["Z"], c["mu"], c["vs"][0]
    Z2 = np.array(Z)
    Z2[c["p"].dt_idx] *= 1.5
    ev = evaluator(c)
    try:
        first = ev.reduced_hessian_product(Z, v, R.SIGMA, mu)
        B = np.ones((c["p"].N, 1, c["p"].integrators[0].x_dim))
        kept_solve = ev.dynamics_solve(Z, B)                       # the single-integrator solves' point: this one is dropped
        phi = ev.feasible_merit(Z2, R.SIGMA, mu)
        assert np.isfinite(phi)
        ev.profile_enable(True)
        ev.profile_reset()
        second = ev.reduced_hessian_product(Z, v, R.SIGMA, mu)
        assert np.array_equal(first, second)
        assert launches(ev, "dynsolve_tree", "bgemm", "chain64") == (0, 0, 0), "the solves', the reduced and the Hessian point are kept"
        assert launches(ev, "hess_product") == (1,), "the product launch alone"
        ev.profile_reset()
        assert np.array_equal(ev.dynamics_solve(Z, B), kept_solve)
        assert launches(ev, "dynsolve_tree")[0] > 0, "like dto_rollout, the call drops dto_dynamics_solve's kept tree"
        ev.profile_enable(False)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------- refusals
def _raw_calls(ev, Z, mu):
    """the two host-pointer entry points through ctypes with NaN-filled outputs: (rc, text, outputs) each"""
    import ctypes as C
    lib, dp = dto_amd.load_library(), dto_amd.capi.c_double_p
    Zc = np.array(Z)
    Zf, g, phi = np.full(ev.n_variables, np.nan), np.full(max(ev.n_constraints, 1), np.nan), C.c_double(np.nan)
    rc1 = lib.dto_feasible_trajectory(ev.handle, Zc.ctypes.data_as(dp), Zf.ctypes.data_as(dp))
    said1 = lib.dto_last_error(ev.handle).decode() if rc1 else ""
    Zf2 = np.full(ev.n_variables, np.nan)
    rc2 = lib.dto_feasible_merit(ev.handle, Zc.ctypes.data_as(dp), 1.0, None if mu is None else np.array(mu).ctypes.data_as(dp),
                                 C.byref(phi), Zf2.ctypes.data_as(dp), g.ctypes.data_as(dp))
    said2 = lib.dto_last_error(ev.handle).decode() if rc2 else ""
    return (rc1, said1, Zf), (rc2, said2, (phi.value, Zf2, g))


def test_refusals_name_the_reason_and_leave_the_handle_usable():
    import ctypes as C
    c = case("scaled_12x9+con")
    Z, mu = c["Z"], c["mu"]
    ev = dto_amd.Evaluator(c["pe"], k_lo=1, k_hi=3)                # a sharded handle
    try:
        (rc1, said1, Zf), (rc2, said2, (phi, Zf2, g)) = _raw_calls(ev, Z, None)
        assert rc1 != 0 and "dto_feasible_trajectory needs an unsharded handle" in said1 and np.isnan(Zf).all()
        assert rc2 != 0 and "dto_feasible_merit needs an unsharded handle" in said2
        assert np.isnan(phi) and np.isnan(Zf2).all() and np.isnan(g).all()
        gg = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(gg, Z)
        assert not np.isnan(gg).any()
    finally:
        ev.close()
    p = O.make_external_integrator_problem()                      # a host-evaluated integrator
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        with pytest.raises(dto_amd.EngineError, match="dto_feasible_trajectory: .*evaluated on the host"):
            ev.feasible_trajectory_engine(p.Z0)
        with pytest.raises(dto_amd.EngineError, match="dto_feasible_merit: .*evaluated on the host"):
            ev.feasible_merit(p.Z0)
        gg = np.full(ev.n_constraints, np.nan); ev.eval_constraint(gg, p.Z0)
        assert not np.isnan(gg).any()
    finally:
        ev.close()
    p = O.make_closure_problem()                                  # host-evaluated constraint and objective: the merit alone refuses
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        with pytest.raises(dto_amd.EngineError, match="dto_feasible_merit: the handle holds host-evaluated terms"):
            ev.feasible_merit(p.Z0)
        assert np.array_equal(ev.feasible_trajectory_engine(p.Z0), ev.feasible_trajectory(p.Z0)), "the trajectory needs no such term"
        assert np.isfinite(ev.eval_objective(p.Z0))
    finally:
        ev.close()
    ev = evaluator(c)                                              # missing arguments
    try:
        lib, dp = dto_amd.load_library(), dto_amd.capi.c_double_p
        Zc, Zf, phi = np.array(Z), np.full(ev.n_variables, np.nan), C.c_double(np.nan)
        assert lib.dto_feasible_trajectory(ev.handle, Zc.ctypes.data_as(dp), None) != 0
        assert "NULL" in lib.dto_last_error(ev.handle).decode()
        assert lib.dto_feasible_trajectory(ev.handle, None, Zf.ctypes.data_as(dp)) != 0
        assert "NULL" in lib.dto_last_error(ev.handle).decode() and np.isnan(Zf).all()
        assert lib.dto_feasible_merit(ev.handle, Zc.ctypes.data_as(dp), 1.0, None, None, Zf.ctypes.data_as(dp), None) != 0
        assert "phi" in lib.dto_last_error(ev.handle).decode() and np.isnan(Zf).all()
        assert lib.dto_feasible_trajectory_dev(ev.handle, None, None, None) != 0
        assert "NULL" in lib.dto_last_error(ev.handle).decode()
        assert lib.dto_feasible_merit_dev(ev.handle, None, 1.0, None, None, None, None, None) != 0
        assert "NULL" in lib.dto_last_error(ev.handle).decode()
        (rc1, _, Zf), (rc2, _, (phi, Zf2, g)) = _raw_calls(ev, Z, mu)   # the handle stays usable
        m = merits("scaled_12x9+con")
        assert rc1 == 0 and rc2 == 0 and np.array_equal(Zf, m["traj"]) and np.array_equal(Zf2, m["traj"]) and np.array_equal(g, m["g"])
        assert phi == merit_in_numpy(1.0, m["f"], np.asarray(mu), m["g"], c["n_dyn"])
    finally:
        ev.close()
