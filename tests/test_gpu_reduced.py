"""GPU: the reduced-space operators (dto_reduced_gradient / dto_reduced_hessian_product and their _dev forms, csrc/dto_reduced.hip).

Two references.  The COMPOSITION (reduced_cases.compose_*): the header's steps written with the Evaluator's existing public methods
and NumPy indexing -- the operators must return its bits, which pins the packers (any index slip changes bits) and the promise that
the routines inside are unchanged.  The DENSE REFERENCE (reduced_cases.dense_reference): T' g and T' H T v from the oracle alone, held
to the bar stated in reduced_cases.py, every factor of which comes from the reference.  Outputs are pre-filled with NaN by the mirror,
so a missing writer shows.  The largest errors seen are in DESIGN 4.27."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import reduced_cases as R
from helpers import rel_err, to_engine

pytestmark = pytest.mark.gpu


def device_arrays(*arrays):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays], torch.cuda.current_stream(dev).cuda_stream


def launches(ev, *names):
    return tuple(ev.profile_get(n)[1] for n in names)


def evaluator(c, **kw):
    return dto_amd.Evaluator(c["pe"], **dict(c["kw"], **kw))


@functools.lru_cache(maxsize=None)
def results(name):
    """engine and composition at the case's point, sigma = SIGMA and the case's mu: computed once per case on handles of their own"""
    c = R.case(name)
    p, Z, mu = c["p"], c["Z"], c["mu"]
    ev = evaluator(c)
    try:
        ys = [ev.reduced_hessian_product(Z, v, R.SIGMA, mu) for v in c["vs"]]     # a product first: it computes the point itself
        r, lam = ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu, costates=True)
        r1 = ev.reduced_lagrangian_gradient(Z)                                    # sigma = 1, mu = None
    finally:
        ev.close()
    ev = evaluator(c)
    try:
        rc, lamc, mut = R.compose_gradient(ev, p, Z, R.SIGMA, mu)
        ysc = [R.compose_product(ev, p, Z, R.SIGMA, mu, v, mut=mut) for v in c["vs"]]
        r1c = ev.reduced_gradient(Z)
    finally:
        ev.close()
    return dict(ys=ys, r=r, lam=lam, r1=r1, rc=rc, lamc=lamc, ysc=ysc, r1c=r1c)


# ------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("name", R.CASES)
def test_bit_identity_with_the_composition(name):
    g = results(name)
    assert not np.isnan(g["r"]).any() and not np.isnan(g["lam"]).any()
    assert np.array_equal(g["r"], g["rc"]) and np.array_equal(g["lam"], g["lamc"])
    for y, yc in zip(g["ys"], g["ysc"]):
        assert not np.isnan(y).any() and np.array_equal(y, yc)
    assert np.array_equal(g["r1"], g["r1c"]), "sigma = 1, mu = None: Evaluator.reduced_gradient bit for bit"


# ----------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", R.CASES)
def test_values_against_the_dense_reference(name):
    c, g = R.case(name), results(name)
    ref = c["ref"]
    eg, bg = float(np.linalg.norm(g["r"] - ref["r_ref"])), R.gradient_bar(ref, c["levels"])
    print(name, "gradient error", eg, "bar", bg, "relative", eg / float(np.linalg.norm(ref["r_ref"])), "||T||", ref["nT"], "||H||", ref["nH"],
          "||g||", ref["ng"])
    assert eg <= bg
    for v, y, yr in zip(c["vs"], g["ys"], c["ys"]):
        e, b, k = float(np.linalg.norm(y - yr)), R.product_bar(ref, v), R.kappa(ref, v)
        print(name, "product error", e, "bar", b, "relative", e / float(np.linalg.norm(yr)), "kappa", k)
        assert k <= R.KAPPA_CAP, "the case is too ill-conditioned for its bar: change its seed"
        assert e <= b
        assert np.all(y[ref["S"]] == 0.0)


# ---------------------------------------------------------------------------------------------------- central differences
@pytest.mark.parametrize("name", ["scaled_12x9+con", "tdb_order1"])
def test_central_differences_through_the_engine(name):
    c = R.case(name)
    p, mu = c["p"], c["mu"]
    rng = np.random.default_rng(29)
    ev = evaluator(c)
    try:
        Zs = ev.feasible_trajectory(c["Z"])
        h = 1e-5
        for trial in range(3):
            d1, d2 = R.free_direction(p, rng), R.free_direction(p, rng)
            an = float(d2 @ ev.reduced_hessian_product(Zs, d1, R.SIGMA, mu))
            rp = ev.reduced_lagrangian_gradient(ev.feasible_trajectory(Zs + h * d1), R.SIGMA, mu)
            rm = ev.reduced_lagrangian_gradient(ev.feasible_trajectory(Zs - h * d1), R.SIGMA, mu)
            fd = float(d2 @ (rp - rm)) / (2.0 * h)
            rel = abs(an - fd) / max(abs(an), abs(fd))
            print(name, "pair", trial, "analytic", an, "central difference", fd, "relative", rel)
            assert rel <= 1e-6, (name, trial, rel)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------- symmetry and linearity
@pytest.mark.parametrize("name", ["scaled_40x6+con", "three_level_40x6", "tdb_order1"])
def test_symmetry_and_linearity(name):
    """the bars of test_symmetry_and_linearity in test_gpu_hessian_product.py (1e-12), scaled by ||T||_2^2 from the dense reference"""
    c = R.case(name)
    p, Z, mu, S = c["p"], c["Z"], c["mu"], c["ref"]["S"]
    scale = 1e-12 * c["ref"]["nT"] ** 2
    rng = np.random.default_rng(4)
    ev = evaluator(c)
    try:
        u, v, w = (rng.standard_normal(ev.n_variables) for _ in range(3))
        clean = [np.where(np.isin(np.arange(x.size), S), 0.0, x) for x in (u, v, w)]
        for x in (u, v, w):
            x[S] = np.nan      # the S entries of v are not read
        Hu, Hv, Hw = (ev.reduced_hessian_product(Z, x, R.SIGMA, mu) for x in (u, v, w))
        for y in (Hu, Hv, Hw):
            assert not np.isnan(y).any() and np.all(y[S] == 0.0)
        a, b = float(clean[0] @ Hv), float(clean[1] @ Hu)
        print(name, "<u, Hv>", a, "<v, Hu>", b, "difference", abs(a - b), "bar", scale * max(1.0, abs(a)))
        assert abs(a - b) <= scale * max(1.0, abs(a))
        al, be = 0.37, -1.9
        Hc = ev.reduced_hessian_product(Z, al * v + be * w, R.SIGMA, mu)
        print(name, "linearity", rel_err(Hc, al * Hv + be * Hw), "bar", scale)
        assert rel_err(Hc, al * Hv + be * Hw) <= scale
    finally:
        ev.close()


# ------------------------------------------------------------------------------------- pointer families, repeats, new points
def test_both_pointer_families_repeated_calls_and_a_rebuilt_point_are_bit_identical():
    import torch
    name = "scaled_40x6+con"
    c, g = R.case(name), results(name)
    p, Z, mu, v = c["p"], c["Z"], c["mu"], c["vs"][0]
    N, D = p.N, sum(it.x_dim for it in p.integrators)
    ev = evaluator(c)
    try:
        (dZ, dmu, dv), st = device_arrays(Z, mu, v)

        def dev_product(dZ_, sigma, dmu_, dv_):
            dy = torch.full((ev.n_variables,), float("nan"), dtype=torch.float64, device=dZ.device)
            ev.reduced_hessian_product_dev(dZ_.data_ptr(), sigma, dmu_.data_ptr() if dmu_ is not None else 0, dv_.data_ptr(), dy.data_ptr(), stream=st)
            torch.cuda.synchronize()
            return dy.cpu().numpy()

        def dev_gradient(dZ_, sigma, dmu_):
            dg = torch.full((ev.n_variables,), float("nan"), dtype=torch.float64, device=dZ.device)
            dl = torch.full((N, D), float("nan"), dtype=torch.float64, device=dZ.device)
            ev.reduced_gradient_dev(dZ_.data_ptr(), sigma, dmu_.data_ptr() if dmu_ is not None else 0, dg.data_ptr(), dl.data_ptr(), stream=st)
            torch.cuda.synchronize()
            return dg.cpu().numpy(), dl.cpu().numpy()

        y_dev = dev_product(dZ, R.SIGMA, dmu, dv)                        # device pointers first, at a new point
        assert np.array_equal(y_dev, g["ys"][0])
        assert np.array_equal(dev_product(dZ, R.SIGMA, dmu, dv), y_dev)   # the cached point
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, mu), y_dev)   # host pointers: another dZ, the same bits
        rg, rl = dev_gradient(dZ, R.SIGMA, dmu)
        assert np.array_equal(rg, g["r"]) and np.array_equal(rl, g["lam"])
        assert np.array_equal(ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu), g["r"])
        rg0, _ = dev_gradient(dZ, 1.0, None)                              # mu = NULL on device pointers; dlam may be NULL too
        assert np.array_equal(rg0, g["r1"])
        dg = torch.full((ev.n_variables,), float("nan"), dtype=torch.float64, device=dZ.device)
        ev.reduced_gradient_dev(dZ.data_ptr(), 1.0, 0, dg.data_ptr(), 0, stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(dg.cpu().numpy(), g["r1"])
        ev.set_option("overlap_sweep", 0)                                 # dto_set_option: every kept point is rebuilt
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, mu), y_dev), "rebuilt and cached give the same bits"
        ev.set_option("overlap_sweep", 1)
        # one ulp in one timestep, in one control, in sigma, in one mu entry: a new point each, with the composition's bits at the
        # changed input.  The timestep scales its interval's generator, sigma scales grad f and the objective's Hessian, the mu entry
        # weighs the norm constraint's gradient and Hessian: gradient AND product move.  du, the control proper of this problem, enters
        # the dynamics linearly (u_{k+1} = u_k + dt du_k) and no objective term: the Jacobian entry it meets is dt, the Hessian entry -1,
        # so neither operator depends on it -- its ulp starts a new point (the kept one must not be served) with unchanged values.
        n_dyn, dt2, du2 = c["n_dyn"], 2 * p.z + p.dt_idx, 2 * p.z + p.integrators[1].xdot_off
        Zt = np.array(Z); Zt[dt2] = np.nextafter(Zt[dt2], np.inf)
        Zc = np.array(Z); Zc[du2] = np.nextafter(Zc[du2], np.inf)
        mu2 = np.array(mu); mu2[n_dyn + 1] = np.nextafter(mu2[n_dyn + 1], np.inf)
        ev.profile_enable(True)
        for what, (Za, sa, ma, moves) in dict(timestep=(Zt, R.SIGMA, mu, True), control=(Zc, R.SIGMA, mu, False),
                                              sigma=(Z, np.nextafter(R.SIGMA, 1.0), mu, True), mu=(Z, R.SIGMA, mu2, True)).items():
            ev.reduced_hessian_product(Z, v, R.SIGMA, mu)
            ev.profile_reset()
            y2 = ev.reduced_hessian_product(Za, v, sa, ma)
            assert launches(ev, "reduced_pack")[0] > 6, (what, "a new point computes the gradient's quantities")
            r2 = ev.reduced_lagrangian_gradient(Za, sa, ma)
            ev2 = evaluator(c)
            try:
                r2c, _, mut = R.compose_gradient(ev2, p, Za, sa, ma)
                y2c = R.compose_product(ev2, p, Za, sa, ma, v, mut=mut)
            finally:
                ev2.close()
            assert np.array_equal(r2, r2c) and np.array_equal(y2, y2c), what
            print(what, "gradient entries moved", int(np.sum(r2 != g["r"])), "product entries moved", int(np.sum(y2 != y_dev)))
            assert np.array_equal(r2, g["r"]) != moves, (what, "gradient")
            assert np.array_equal(y2, y_dev) != moves, (what, "product")
        ev.profile_enable(False)
    finally:
        ev.close()


# ----------------------------------------------------------------------------------------------------- launch accounting
@pytest.mark.parametrize("name", ["scaled_40x6", "scaled_70x5", "scaled_40x6+con"], ids=["one_launch_chain", "general_path", "with_mu"])
def test_launch_accounting(name):
    import torch
    c, g = R.case(name), results(name)
    p, Z, mu, (v0, v1) = c["p"], c["Z"], c["mu"], c["vs"]
    D = sum(it.x_dim for it in p.integrators)
    ev = evaluator(c)
    try:
        (dZ,), st = device_arrays(Z)
        dvals = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dZ.device)
        ev.profile_enable(True)
        ev.eval_jacobian_dev(dZ.data_ptr(), dvals.data_ptr(), stream=st)
        torch.cuda.synchronize()
        jac = launches(ev, "chain64", "bgemm")
        assert sum(jac) > 0
        ev.profile_reset()
        y0 = ev.reduced_hessian_product(Z, v0, R.SIGMA, mu)                           # a new point
        print(name, "new point: chain64, bgemm", launches(ev, "chain64", "bgemm"), "of one Jacobian", jac, "reduced_pack",
              launches(ev, "reduced_pack"), "hess_product", launches(ev, "hess_product"))
        assert launches(ev, "chain64", "bgemm") == jac, "the chain runs as often as in one eval_jacobian_dev"
        assert launches(ev, "hess_product") == (2,)                                   # the gather and the product
        assert np.array_equal(y0, g["ys"][0])
        packs = []
        for v, want in ((v1, g["ys"][1]), (v0, g["ys"][0])):                          # second and third product at the same point
            ev.profile_reset()
            y = ev.reduced_hessian_product(Z, v, R.SIGMA, mu)
            assert launches(ev, "chain64", "bgemm", "dynsolve_tree") == (0, 0, 0)
            assert launches(ev, "hess_product") == (1,), "the product launch alone: mu~ is bit-identical, the Hessian is kept"
            packs.append(launches(ev, "reduced_pack")[0])
            assert np.array_equal(y, want)
        assert packs == [6, 6], packs
        assert ev.profile_get("reduced_pack")[2] > 0, "bytes as executed"
        # an interleaved H v at another mu takes the Hessian slab: one re-assembly, the same bits
        other = np.random.default_rng(1).standard_normal(ev.n_constraints)
        q = np.full(ev.n_variables, np.nan)
        ev.eval_hessian_lagrangian_product(q, Z, v0, R.SIGMA, other)
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, v0, R.SIGMA, mu), g["ys"][0])
        assert launches(ev, "hess_product") == (2,) and launches(ev, "chain64", "bgemm", "dynsolve_tree") == (0, 0, 0)
        assert launches(ev, "reduced_pack") == (6,)
        # the routines the operators are made of, called in between, keep their behaviour
        B = np.random.default_rng(2).standard_normal((p.N, 1, D))
        ev2 = evaluator(c)
        try:
            want_solve = ev2.dynamics_solve_all(Z, B)
            ev2.profile_enable(True)
            want_roll = ev2.rollout(Z)
            roll_launches = launches(ev2, "rollout", "rollout_tree", "chain64", "bgemm")
            ev2.profile_enable(False)
            q2 = np.full(ev.n_variables, np.nan); ev2.eval_hessian_lagrangian_product(q2, Z, v0, R.SIGMA, other)
        finally:
            ev2.close()
        ev.profile_reset()
        assert np.array_equal(ev.dynamics_solve_all(Z, B), want_solve)
        assert launches(ev, "chain64", "bgemm", "dynsolve_tree") == (0, 0, 0), "the solves' kept point is the operators' too"
        ev.profile_reset()
        assert np.array_equal(ev.rollout(Z), want_roll)
        assert launches(ev, "rollout", "rollout_tree", "chain64", "bgemm") == roll_launches, "dto_rollout's launches on a handle of its own"
        q = np.full(ev.n_variables, np.nan); ev.eval_hessian_lagrangian_product(q, Z, v0, R.SIGMA, other)
        assert np.array_equal(q, q2)
        ev.profile_reset()
        ev.eval_hessian_lagrangian_product(q, Z, v1, R.SIGMA, other)
        assert launches(ev, "hess_product") == (1,), "dto_eval_hessian_product keeps its own point"
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, v1, R.SIGMA, mu), g["ys"][1])
        assert launches(ev, "dynsolve_tree") == (0,) and launches(ev, "reduced_pack") == (6,)
        ev.profile_reset()
        assert np.array_equal(ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu), g["r"])
        assert launches(ev, "reduced_pack", "all") == (0, 0), "a gradient at the kept point copies its result"
        ev.profile_enable(False)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_reason_and_leave_the_handle_usable():
    c = R.case("scaled_12x9")
    Z, v = c["Z"], c["vs"][0]
    ev = evaluator(c, eval_hessian=False)
    try:
        with pytest.raises(dto_amd.EngineError, match="dto_reduced_hessian_product: handle was created with eval_hessian = 0"):
            ev.reduced_hessian_product(Z, v)
        assert np.array_equal(ev.reduced_lagrangian_gradient(Z), results("scaled_12x9")["r1"]), "the gradient still works"
    finally:
        ev.close()
    p = O.make_closure_problem()
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        with pytest.raises(dto_amd.EngineError, match="host-evaluated terms"):
            ev.reduced_lagrangian_gradient(p.Z0)
        with pytest.raises(dto_amd.EngineError, match="host-evaluated terms"):
            ev.reduced_hessian_product(p.Z0, np.ones(ev.n_variables))
        assert np.isfinite(ev.eval_objective(p.Z0))
    finally:
        ev.close()
    p = O.make_external_integrator_problem()
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        with pytest.raises(dto_amd.EngineError, match="dto_reduced_gradient: .*evaluated on the host"):
            ev.reduced_lagrangian_gradient(p.Z0)
        with pytest.raises(dto_amd.EngineError, match="dto_reduced_hessian_product: .*evaluated on the host"):
            ev.reduced_hessian_product(p.Z0, np.ones(ev.n_variables))
        gg = np.full(ev.n_constraints, np.nan); ev.eval_constraint(gg, p.Z0)
        assert not np.isnan(gg).any()
    finally:
        ev.close()
    ev = dto_amd.Evaluator(c["pe"], k_lo=1, k_hi=3)
    try:
        with pytest.raises(dto_amd.EngineError, match="dto_reduced_gradient needs an unsharded handle"):
            ev.reduced_lagrangian_gradient(Z)
        with pytest.raises(dto_amd.EngineError, match="dto_reduced_hessian_product needs an unsharded handle"):
            ev.reduced_hessian_product(Z, v)
        gg = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(gg, Z)
        assert not np.isnan(gg).any()
    finally:
        ev.close()
    ev = evaluator(c)
    try:
        lib, dp = dto_amd.load_library(), dto_amd.capi.c_double_p
        Zc, out = np.array(Z), np.full(ev.n_variables, np.nan)
        assert lib.dto_reduced_hessian_product(ev.handle, Zc.ctypes.data_as(dp), 1.0, None, None, out.ctypes.data_as(dp)) != 0
        assert "NULL" in lib.dto_last_error(ev.handle).decode() and np.isnan(out).all()
        assert lib.dto_reduced_hessian_product(ev.handle, Zc.ctypes.data_as(dp), 1.0, None, np.array(v).ctypes.data_as(dp), None) != 0
        assert "NULL" in lib.dto_last_error(ev.handle).decode()
        assert lib.dto_reduced_gradient(ev.handle, Zc.ctypes.data_as(dp), 1.0, None, None, None) != 0
        assert "NULL" in lib.dto_last_error(ev.handle).decode()
        assert lib.dto_reduced_hessian_product_dev(ev.handle, None, 1.0, None, None, None, None) != 0
        assert "NULL" in lib.dto_last_error(ev.handle).decode()
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, c["mu"]), results("scaled_12x9")["ys"][0])   # the handle stays usable
    finally:
        ev.close()


# ----------------------------------------------------------------------------------------------- the other product route
def test_time_dependent_matrix_free_products_give_the_same_values():
    """tdb_matrix_free_products = 1: J w / J' w without the value slab; another summation order, so values to the bar, not bits"""
    name = "tdb_order1"
    c, g = R.case(name), results(name)
    ref = c["ref"]
    ev = evaluator(c)
    try:
        ev.set_option("tdb_matrix_free_products", 1)
        r = ev.reduced_lagrangian_gradient(c["Z"], R.SIGMA, c["mu"])
        eg = float(np.linalg.norm(r - ref["r_ref"]))
        print(name, "matrix-free: gradient error", eg, "bar", R.gradient_bar(ref, c["levels"]), "against the slab route",
              float(np.linalg.norm(r - g["r"])))
        assert eg <= R.gradient_bar(ref, c["levels"])
        for v, yr, ys in zip(c["vs"], c["ys"], g["ys"]):
            y = ev.reduced_hessian_product(c["Z"], v, R.SIGMA, c["mu"])
            e = float(np.linalg.norm(y - yr))
            print(name, "matrix-free: product error", e, "bar", R.product_bar(ref, v), "against the slab route", float(np.linalg.norm(y - ys)))
            assert e <= R.product_bar(ref, v)
            assert float(np.linalg.norm(y - ys)) <= R.product_bar(ref, v)
    finally:
        ev.close()
