"""GPU: the reduced-space operators with the option "reduced_input_store" = 1 (csrc/dto_input_plan.h, the k_red_input_* kernels of
csrc/dto_reduced.hip): J v^ and J' w taken from input blocks kept with the whole-dynamics solves' point.

BITS against the store route's composition (reduced_input_cases): the header's steps with the Evaluator's public methods, the two
Jacobian products replaced by the stated sums over entries cut from the same Evaluator's public Jacobian values.  VALUES against the
dense reference of reduced_cases with its bars unchanged.  Then the properties the header promises, the stale-store hazard, the launch
accounting and switching the option on one handle.  Every case runs on handles of its own.  The largest errors seen are in DESIGN 4.28."""
import functools

import numpy as np
import pytest

import dto_amd
import reduced_cases as R
import reduced_input_cases as RI

pytestmark = pytest.mark.gpu

# every name under which a Jacobian evaluation, a propagator chain, a sweep or a Jacobian product can count
JACOBIAN_NAMES = ("expmv", "expmv_adjoint", "jac_product", "tdb_product", "chain64", "bgemm", "bgemm_horner", "bgemm_square", "bgemm_plain",
                  "basis", "basis_k", "basis_multi", "zero_fill", "build_A", "assembly", "share", "tdb_mfma", "tdb_kron", "dynsolve_tree")
# what one Jacobian evaluation launches
JACOBIAN_EVAL = ("expmv",) + JACOBIAN_NAMES[4:-1]


def device_arrays(*arrays):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays], torch.cuda.current_stream(dev).cuda_stream


def launches(ev, *names):
    return tuple(ev.profile_get(n)[1] for n in names)


def evaluator(c, store=1, **kw):
    ev = dto_amd.Evaluator(c["pe"], **dict(c["kw"], **kw))
    if store is not None:
        ev.set_option(RI.OPTION, store)
    return ev


def n_gathers(p):
    return sum(1 for f in RI.free_inputs(p)[0] if f)


@functools.lru_cache(maxsize=None)
def results(name):
    """the store route and its composition at the case's point, sigma = SIGMA and the case's mu; the default route beside them"""
    c = R.case(name)
    p, Z, mu = c["p"], c["Z"], c["mu"]
    out = {}
    for key, store in (("", 1), ("default_", 0)):
        ev = evaluator(c, store)
        try:
            out[key + "ys"] = [ev.reduced_hessian_product(Z, v, R.SIGMA, mu) for v in c["vs"]]   # a product first: it computes the point
            out[key + "r"], out[key + "lam"] = ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu, costates=True)
        finally:
            ev.close()
    ev = evaluator(c, None)
    try:
        S = RI.store_from_jacobian(ev, p, Z)
        out["rc"], out["lamc"], mut = RI.compose_gradient(ev, p, Z, R.SIGMA, mu, S)
        out["ysc"] = [RI.compose_product(ev, p, Z, R.SIGMA, mu, v, S, mut) for v in c["vs"]]
    finally:
        ev.close()
    return out


# ------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("name", R.CASES + [RI.N2_CASE])
def test_bit_identity_with_the_store_routes_composition(name):
    g = results(name)
    assert not np.isnan(g["r"]).any() and not np.isnan(g["lam"]).any()
    print(name, "gradient entries that differ", int(np.sum(g["r"] != g["rc"])), "largest", float(np.max(np.abs(g["r"] - g["rc"]))))
    assert np.array_equal(g["lam"], g["lamc"]), "the costates come from the unchanged adjoint solve"
    assert np.array_equal(g["r"], g["rc"])
    for y, yc in zip(g["ys"], g["ysc"]):
        print(name, "product entries that differ", int(np.sum(y != yc)), "largest", float(np.max(np.abs(y - yc))))
        assert not np.isnan(y).any() and np.array_equal(y, yc)


# ----------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", R.CASES)
def test_values_against_the_dense_reference(name):
    c, g = R.case(name), results(name)
    ref = c["ref"]
    eg, bg = float(np.linalg.norm(g["r"] - ref["r_ref"])), R.gradient_bar(ref, c["levels"])
    print(name, "gradient error", eg, "bar", bg, "relative", eg / float(np.linalg.norm(ref["r_ref"])), "between the routes",
          float(np.linalg.norm(g["r"] - g["default_r"])))
    assert eg <= bg
    assert np.array_equal(g["lam"], g["default_lam"])
    for v, y, yd, yr in zip(c["vs"], g["ys"], g["default_ys"], c["ys"]):
        e, b, k = float(np.linalg.norm(y - yr)), R.product_bar(ref, v), R.kappa(ref, v)
        print(name, "product error", e, "bar", b, "relative", e / float(np.linalg.norm(yr)), "kappa", k, "between the routes",
              float(np.linalg.norm(y - yd)), "relative", float(np.linalg.norm(y - yd)) / float(np.linalg.norm(yr)))
        assert k <= R.KAPPA_CAP, "the case is too ill-conditioned for its bar: change its seed"
        assert e <= b
        assert float(np.linalg.norm(y - yd)) <= b, "the two routes differ by summation order alone"
        assert np.all(y[ref["S"]] == 0.0)


# ------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("name", ["scaled_70x5", "tdb_order1"])
def test_a_nan_in_a_dependent_entry_of_v_reaches_nothing(name):
    c, g = R.case(name), results(name)
    S = c["ref"]["S"]
    ev = evaluator(c)
    try:
        for v, want in zip(c["vs"], g["ys"]):
            vn = np.array(v)
            vn[S] = np.nan
            y = ev.reduced_hessian_product(c["Z"], vn, R.SIGMA, c["mu"])
            assert not np.isnan(y).any() and np.array_equal(y, want), "the S entries of v are not read"
            assert np.all(y[S] == 0.0), "y is zero on S"
    finally:
        ev.close()


def test_both_pointer_families_repeated_calls_and_a_rebuilt_point_are_bit_identical():
    import torch
    name = "scaled_40x6+con"
    c, g = R.case(name), results(name)
    p, Z, mu, v = c["p"], c["Z"], c["mu"], c["vs"][0]
    N, D = p.N, sum(it.x_dim for it in p.integrators)
    ev = evaluator(c)
    try:
        (dZ, dmu, dv), st = device_arrays(Z, mu, v)

        def dev_product():
            dy = torch.full((ev.n_variables,), float("nan"), dtype=torch.float64, device=dZ.device)
            ev.reduced_hessian_product_dev(dZ.data_ptr(), R.SIGMA, dmu.data_ptr(), dv.data_ptr(), dy.data_ptr(), stream=st)
            torch.cuda.synchronize()
            return dy.cpu().numpy()

        y_dev = dev_product()                                             # device pointers first, at a new point
        assert np.array_equal(y_dev, g["ys"][0])
        assert np.array_equal(dev_product(), y_dev)                       # the kept point
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, mu), y_dev)   # host pointers: another dZ, the same bits
        dg = torch.full((ev.n_variables,), float("nan"), dtype=torch.float64, device=dZ.device)
        dl = torch.full((N, D), float("nan"), dtype=torch.float64, device=dZ.device)
        ev.reduced_gradient_dev(dZ.data_ptr(), R.SIGMA, dmu.data_ptr(), dg.data_ptr(), dl.data_ptr(), stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(dg.cpu().numpy(), g["r"]) and np.array_equal(dl.cpu().numpy(), g["lam"])
        assert np.array_equal(ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu), g["r"])
        ev.set_option("overlap_sweep", 0)                                 # dto_set_option: every kept point is rebuilt
        ev.set_option("overlap_sweep", 1)
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, mu), y_dev), "rebuilt and kept give the same bits"
        assert np.array_equal(ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu), g["r"])
        assert np.array_equal(ev.reduced_hessian_product(Z, c["vs"][1], R.SIGMA, mu), g["ys"][1])
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------ stale store
@pytest.mark.parametrize("name", ["scaled_40x6", "tdb_order1"])
def test_a_solve_at_another_point_between_two_products_costs_one_rebuild_and_no_bit(name):
    import torch
    c, g = R.case(name), results(name)
    p, Z, mu, v = c["p"], c["Z"], c["mu"], c["vs"][0]
    D = sum(it.x_dim for it in p.integrators)
    ev = evaluator(c)
    try:
        (dZ,), st = device_arrays(Z)
        dvals = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dZ.device)
        ev.profile_enable(True)
        for _ in range(2):                                                # the second evaluation: nothing is set up any more
            ev.profile_reset()
            ev.eval_jacobian_dev(dZ.data_ptr(), dvals.data_ptr(), stream=st)
            torch.cuda.synchronize()
        one_jacobian = launches(ev, *JACOBIAN_EVAL)
        assert sum(one_jacobian) > 0
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, mu), g["ys"][0])
        other = np.array(Z) * (1.0 + 0.05 * np.random.default_rng(8).standard_normal(Z.size))
        ev.dynamics_solve_all(other, np.ones((p.N, 1, D)))                # the solves' point moves, the store with it; the reduced point stays
        ev.profile_reset()
        y = ev.reduced_hessian_product(Z, v, R.SIGMA, mu)
        print(name, "after a solve elsewhere: entries that differ", int(np.sum(y != g["ys"][0])), "reduced_input, reduced_pack, dynsolve_tree",
              launches(ev, "reduced_input", "reduced_pack", "dynsolve_tree"), "Jacobian", launches(ev, *JACOBIAN_EVAL), "one", one_jacobian)
        assert np.array_equal(y, g["ys"][0]), "the product made the solves' point its own before it read the store"
        assert launches(ev, *JACOBIAN_EVAL) == one_jacobian, "exactly one Jacobian evaluation for the rebuild"
        assert launches(ev, "dynsolve_tree")[0] > 0
        assert launches(ev, "reduced_input", "reduced_pack") == (n_gathers(p) + 2, 2), "the gathers of the rebuild and the two products"
        assert launches(ev, "jac_product", "tdb_product") == (0, 0)
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, mu), g["ys"][0])
        assert launches(ev, "reduced_input", "dynsolve_tree") == (2, 0), "kept again"
        ev.profile_enable(False)
    finally:
        ev.close()


# ----------------------------------------------------------------------------------------------------- launch accounting
@pytest.mark.parametrize("name", ["scaled_70x5", "scaled_40x6+con", "tdb_order1"], ids=["general_path", "one_launch_chain", "time_dependent_slab_route"])
def test_launch_accounting(name):
    import torch
    c, g = R.case(name), results(name)
    p, Z, mu, (v0, v1) = c["p"], c["Z"], c["mu"], c["vs"]
    ev = evaluator(c)
    try:
        (dZ,), st = device_arrays(Z)
        dvals = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dZ.device)
        ev.profile_enable(True)
        ev.eval_jacobian_dev(dZ.data_ptr(), dvals.data_ptr(), stream=st)
        torch.cuda.synchronize()
        jac = launches(ev, "chain64", "bgemm")
        assert name.startswith("tdb") or sum(jac) > 0
        ev.profile_reset()
        y0 = ev.reduced_hessian_product(Z, v0, R.SIGMA, mu)                            # a new point
        print(name, "new point: chain64, bgemm", launches(ev, "chain64", "bgemm"), "of one Jacobian", jac, "reduced_input, reduced_pack",
              launches(ev, "reduced_input", "reduced_pack"))
        assert launches(ev, "chain64", "bgemm") == jac, "the chain runs as often as in one eval_jacobian_dev"
        # the gathers, the gradient's J' w2 and the product's two; the gradient's packers (one more with mu) and the product's two
        assert launches(ev, "reduced_input", "reduced_pack") == (n_gathers(p) + 3, (3 if mu is not None else 2) + 2)
        assert np.array_equal(y0, g["ys"][0])
        for v, want in ((v1, g["ys"][1]), (v0, g["ys"][0])):                           # the kept point
            ev.profile_reset()
            y = ev.reduced_hessian_product(Z, v, R.SIGMA, mu)
            assert np.array_equal(y, want)
            assert launches(ev, *JACOBIAN_NAMES) == (0,) * len(JACOBIAN_NAMES), dict(zip(JACOBIAN_NAMES, launches(ev, *JACOBIAN_NAMES)))
            assert launches(ev, "reduced_input", "reduced_pack", "hess_product") == (2, 2, 1)
            # "all" leaves out the names that feed no other: what it counts is then the H v launch alone, so every launch of the
            # product counts under reduced_input, reduced_pack, hess_product, dynsolve_scan, dynsolve_couple or dynsolve_deriv
            assert launches(ev, "all") == launches(ev, "hess_product")
            assert launches(ev, "rollout", "dynsolve_tree") == (0, 0)
            assert launches(ev, "dynsolve_scan")[0] > 0 and sum(launches(ev, "dynsolve_couple", "dynsolve_deriv")) > 0
        ms, n, nbytes = ev.profile_get("reduced_input")
        assert n == 2 and nbytes > 0 and ms > 0.0, "bytes as executed"
        ev.profile_reset()
        assert np.array_equal(ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu), g["r"])
        assert launches(ev, "reduced_input", "reduced_pack", "all") == (0, 0, 0), "a gradient at the kept point copies its result"
        ev.profile_enable(False)
    finally:
        ev.close()


# -------------------------------------------------------------------------------------------------------------- switching
@pytest.mark.parametrize("name", ["scaled_12x9+con", "tdb_order1"])
def test_switching_the_option_on_one_handle(name):
    c, g = R.case(name), results(name)
    Z, mu, v = c["Z"], c["mu"], c["vs"][0]
    ev = evaluator(c, 1)
    try:
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, mu), g["ys"][0])
        ev.set_option(RI.OPTION, 0)
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, mu), g["default_ys"][0]), "1 -> 0: a fresh default-route handle's bits"
        assert np.array_equal(ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu), g["default_r"])
        ev.set_option(RI.OPTION, 1)
        assert np.array_equal(ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu), g["r"])
        assert np.array_equal(ev.reduced_hessian_product(Z, v, R.SIGMA, mu), g["ys"][0])
    finally:
        ev.close()
    ev = evaluator(c, 1)
    try:
        assert np.array_equal(ev.reduced_hessian_product(Z, c["vs"][1], R.SIGMA, mu), g["ys"][1]), "another fresh handle reproduces the first run"
    finally:
        ev.close()
