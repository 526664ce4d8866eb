"""GPU: block reduced Hessian products Y = T' H(Z; sigma, mu~) T V (dto_projected_hessian_products[_dev]; the block kernels of
csrc/dto_reduced.hip and k_hess_spmm of csrc/dto_hess_product.hip).

BITS: every column against dto_reduced_hessian_product of that column on a handle of its own, on both routes (option
"reduced_input_store" 0 and 1) and for chunk widths 1, 3, 64 and the default.  35 columns make the time-dependent cases (column limit 4)
run 9 chunks and the 12-state cases 3.  VALUES: every column against the dense reference of reduced_cases, its bars unchanged.  The
DENSE MATRIX from unit vectors against the reference's T' H T.  Then the properties the header promises and the launch accounting."""
import functools

import numpy as np
import pytest

import dto_amd
import reduced_cases as R
from helpers import TOL_H, to_engine
from test_gpu_reduced_input import JACOBIAN_NAMES, device_arrays, evaluator, launches

pytestmark = pytest.mark.gpu

N_COLS = 35
BIT_CASES = R.CASES + ["scaled_12x2", "scaled_130x3"]
WIDTHS = (0, 1, 3, 64)
ROUTES = {"store": 1, "default": 0}


DEFAULT_WIDTH = 64   # the engine's choice of chunk width (include/dto_engine.h, "Block products")


@functools.lru_cache(maxsize=None)
def setup(name):
    """R.case for the cases with a dense reference; for the bits-only ones the same record without it"""
    if name in R.CASES:
        return R.case(name)
    p, kw = R.problem(name)
    Z = np.ascontiguousarray(p.Z0, dtype=np.float64)
    Z.setflags(write=False)
    return dict(p=p, pe=to_engine(p), kw=kw, Z=Z, mu=None)


@functools.lru_cache(maxsize=None)
def vectors(name):
    c = setup(name)
    V = np.random.default_rng(1000 + len(name)).standard_normal((N_COLS, c["p"].n_vars))
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def singles(name, store):
    """dto_reduced_hessian_product of every column, on a handle of its own"""
    c, V = setup(name), vectors(name)
    ev = evaluator(c, store)
    try:
        Y = np.stack([ev.reduced_hessian_product(c["Z"], v, R.SIGMA, c["mu"]) for v in V])
    finally:
        ev.close()
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def blocks(name, store):
    """the block product per chunk width, all on one handle (dto_set_option drops the kept points: every call builds its own)"""
    c, V = setup(name), vectors(name)
    ev = evaluator(c, store)
    out = {}
    try:
        for width in WIDTHS:
            ev.set_option("reduced_block_width", width)
            out[width] = ev.reduced_hessian_products(c["Z"], V, R.SIGMA, c["mu"])
    finally:
        ev.close()
    return out


# ------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", BIT_CASES)
def test_every_column_has_the_bits_of_the_single_product_at_every_width(name, route):
    want, got = singles(name, ROUTES[route]), blocks(name, ROUTES[route])
    assert not np.isnan(want).any()
    for width in WIDTHS:
        Y = got[width]
        print(name, route, "width", width, "entries that differ", int(np.sum(Y != want)), "largest", float(np.max(np.abs(Y - want))))
        assert Y.shape == want.shape and not np.isnan(Y).any()
        assert np.array_equal(Y, want), (name, route, width)


# ----------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", R.CASES)
def test_values_against_the_dense_reference(name, route):
    ref, V, Y = R.case(name)["ref"], vectors(name), blocks(name, ROUTES[route])[0]
    worst, kmax = 0.0, 0.0
    for v, y in zip(V, Y):
        k, e, b = R.kappa(ref, v), float(np.linalg.norm(y - R.product_ref(ref, v))), R.product_bar(ref, v)
        worst, kmax = max(worst, e / b), max(kmax, k)
        assert k <= R.KAPPA_CAP, "the column is too ill-conditioned for its bar"
        assert e <= b, (name, route, e, b)
        assert np.all(y[ref["S"]] == 0.0)
    print(name, route, "largest error / bar", worst, "largest kappa", kmax)


# ----------------------------------------------------------------------------------------------------------- dense matrix
@pytest.mark.parametrize("name", ["scaled_12x9+con", "tdb_order1", "structured_16x4"])
def test_the_dense_reduced_hessian_from_unit_vectors(name):
    c = R.case(name)
    ref = c["ref"]
    ev = evaluator(c)
    try:
        Hr, C = ev.reduced_hessian_matrix(c["Z"], R.SIGMA, c["mu"])
    finally:
        ev.close()
    assert np.array_equal(C, ref["C"]) and Hr.shape == (C.size, C.size)
    bar = TOL_H * ref["nT"] ** 2 * ref["nH"] * np.sqrt(C.size)   # the unit vectors' bars (||e_i|| = 1) summed in quadrature
    err, asym = float(np.linalg.norm(Hr - ref["Hr"])), float(np.linalg.norm(Hr - Hr.T))
    print(name, "|C|", C.size, "error", err, "asymmetry", asym, "bar", bar, "||Hr||_F", float(np.linalg.norm(ref["Hr"])))
    assert err <= bar
    assert asym <= 2.0 * bar


# ------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["scaled_70x5", "tdb_order1"])
def test_a_nan_in_the_dependent_entries_of_V_reaches_nothing(name, route):
    c, want = R.case(name), singles(name, ROUTES[route])
    S = c["ref"]["S"]
    Vn = np.array(vectors(name))
    Vn[:, S] = np.nan
    ev = evaluator(c, ROUTES[route])
    try:
        Y = ev.reduced_hessian_products(c["Z"], Vn, R.SIGMA, c["mu"])
    finally:
        ev.close()
    assert not np.isnan(Y).any() and np.array_equal(Y, want), "the S entries of V are not read"
    assert np.all(Y[:, S] == 0.0), "Y is zero on S"


@pytest.mark.parametrize("route", list(ROUTES))
def test_both_pointer_families_a_rebuilt_point_and_a_block_after_a_single_product(route):
    import torch
    name = "scaled_40x6+con"
    c, V, want = R.case(name), vectors(name), singles(name, ROUTES[route])
    Z, mu = c["Z"], c["mu"]
    ev = evaluator(c, ROUTES[route])
    try:
        n = ev.n_variables
        (dZ, dmu, dV), st = device_arrays(Z, mu, V)

        def dev_products():
            dY = torch.full((N_COLS, n), float("nan"), dtype=torch.float64, device=dZ.device)
            ev.reduced_hessian_products_dev(dZ.data_ptr(), R.SIGMA, dmu.data_ptr(), N_COLS, dV.data_ptr(), dY.data_ptr(), stream=st)
            torch.cuda.synchronize()
            return dY.cpu().numpy()

        assert np.array_equal(dev_products(), want)                       # device pointers first, at a new point
        assert np.array_equal(dev_products(), want)                       # the kept point
        assert np.array_equal(ev.reduced_hessian_products(Z, V, R.SIGMA, mu), want)   # host pointers: another dZ, the same bits
        ev.set_option("overlap_sweep", 0)                                 # dto_set_option: every kept point is rebuilt
        ev.set_option("overlap_sweep", 1)
        assert np.array_equal(ev.reduced_hessian_products(Z, V, R.SIGMA, mu), want), "rebuilt and kept give the same bits"
        ev.set_option("overlap_sweep", 0)
        ev.set_option("overlap_sweep", 1)
        assert np.array_equal(ev.reduced_hessian_product(Z, V[2], R.SIGMA, mu), want[2])   # a single product computes the points
        ev.profile_enable(True)
        ev.profile_reset()
        Y = ev.reduced_hessian_products(Z, V, R.SIGMA, mu)                # a block call after it: no new point
        assert np.array_equal(Y, want)
        assert launches(ev, "dynsolve_tree") == (0,), "the solves' point of the single product is the block call's"
        assert launches(ev, "hess_product") == (-(-N_COLS // min(DEFAULT_WIDTH, 40, N_COLS)),), "one launch per chunk (40 states cap it): no gather, so no assembly"
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, V[7], R.SIGMA, mu), want[7])   # and the other way round
        assert launches(ev, "dynsolve_tree", "hess_product") == (0, 1)
        ev.profile_enable(False)
    finally:
        ev.close()


def test_refusals_leave_the_handle_usable():
    name = "scaled_12x9"
    c, V, want = R.case(name), vectors(name), singles(name, 1)
    ev = evaluator(c)
    try:
        n = ev.n_variables
        with pytest.raises(dto_amd.EngineError, match="n_cols = 0"):
            ev.reduced_hessian_products(c["Z"], np.zeros((0, n)), R.SIGMA, c["mu"])
        with pytest.raises(dto_amd.EngineError, match="NULL"):
            ev.reduced_hessian_products_dev(1, R.SIGMA, 0, 2, 0, 1)
        assert np.array_equal(ev.reduced_hessian_products(c["Z"], V[:5], R.SIGMA, c["mu"]), want[:5])
    finally:
        ev.close()


# ----------------------------------------------------------------------------------------------------- launch accounting
@pytest.mark.parametrize("name", ["scaled_70x5", "tdb_order1"])
def test_launch_accounting_on_the_store_route(name):
    c, V, want = R.case(name), vectors(name), singles(name, 1)
    Z, mu = c["Z"], c["mu"]
    ev = evaluator(c)
    try:
        ev.set_option("reduced_block_width", 4)
        assert np.array_equal(ev.reduced_hessian_products(Z, V[:2], R.SIGMA, mu), want[:2])   # the points
        ev.profile_enable(True)
        for n_cols, chunks in ((4, 1), (9, 3)):
            ev.profile_reset()
            Y = ev.reduced_hessian_products(Z, V[:n_cols], R.SIGMA, mu)
            assert np.array_equal(Y, want[:n_cols])
            print(name, n_cols, "columns: reduced_input, reduced_pack, hess_product", launches(ev, "reduced_input", "reduced_pack", "hess_product"))
            assert launches(ev, "reduced_input", "reduced_pack", "hess_product") == (2 * chunks, 2 * chunks, chunks)
            assert launches(ev, *JACOBIAN_NAMES) == (0,) * len(JACOBIAN_NAMES), dict(zip(JACOBIAN_NAMES, launches(ev, *JACOBIAN_NAMES)))
            assert launches(ev, "dynsolve_scan")[0] > 0
            for key in ("reduced_input", "reduced_pack", "hess_product"):
                assert ev.profile_get(key)[2] > 0, "bytes as executed"
        ev.profile_enable(False)
    finally:
        ev.close()


@pytest.mark.parametrize("name", ["scaled_70x5", "tdb_order1"])
def test_launch_accounting_on_the_default_route(name):
    c, V, want = R.case(name), vectors(name), singles(name, 0)
    Z, mu = c["Z"], c["mu"]
    ev = evaluator(c, 0)
    try:
        assert np.array_equal(ev.reduced_hessian_product(Z, V[0], R.SIGMA, mu), want[0])      # the points
        ev.profile_enable(True)
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, V[1], R.SIGMA, mu), want[1])
        one = launches(ev, *JACOBIAN_NAMES)
        assert sum(one) > 0 and launches(ev, "reduced_pack", "dynsolve_tree") == (6, 0)
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_products(Z, V[:3], R.SIGMA, mu), want[:3])
        print(name, "Jacobian-product launches of one product", dict(zip(JACOBIAN_NAMES, one)), "of a block of 3", launches(ev, *JACOBIAN_NAMES))
        assert launches(ev, "reduced_pack", "hess_product", "reduced_input") == (6, 1, 0), "the six packers in block form, once"
        assert launches(ev, *JACOBIAN_NAMES) == tuple(3 * k for k in one), "J v^ and J' w once per column"
        ev.profile_enable(False)
    finally:
        ev.close()
