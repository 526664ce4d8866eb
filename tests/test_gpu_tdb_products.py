"""GPU: matrix-free J w / J' w of device TimeDependentBilinearIntegrators (option "tdb_matrix_free_products" = 1; the product
modes of csrc/dto_tdb.hip, 1..64 states, and csrc/dto_tdb_mfma.hip, 65..256 states).

Expected values, both independent of the engine: up to 64 states the oracle's eval_constraint_jacobian_product /
eval_constraint_jacobian_transpose_product of O.make_tdb_problem(...); above, the Jacobian values of tdb_large_cases.reference(...)
contracted with np.add.at.  The bar is helpers.TOL, 1e-10 max(1, |ref|), the project's bar for first-order quantities.  Outputs are
filled with NaN beforehand so that a missing writer shows.  Shapes are n, m, order, substeps, n_mods, N."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import tdb_large_cases as L
from helpers import TOL, rel_err, to_engine
from test_gpu_jacobian_products import dev_products, host_products

pytestmark = pytest.mark.gpu

OPTION = "tdb_matrix_free_products"
# k_tdb: the make_tdb_problem defaults; one state, no drive-free modulation; below and at the value kernel's adjoint threshold of 12;
# more than one pass of 256 threads over the columns' rows; the cap
SCALAR = [(4, 2, 1, 16, 2, 6), (1, 1, 0, 4, 0, 3), (11, 2, 0, 4, 1, 3), (12, 2, 1, 4, 2, 3), (24, 3, 1, 4, 2, 3), (64, 1, 1, 2, 2, 3)]
# k_tdb_mfma: 31 padded rows on the 32-row tile; ragged 64-row tiles; exact tiles, no modulation; the cap
MFMA = [(65, 1, 0, 2, 2, 3), (72, 2, 1, 4, 2, 3), (128, 2, 1, 3, 0, 3), (256, 2, 1, 2, 2, 3)]


def _problem(n, m, order, substeps, n_mods, N, with_derivative=False):
    if (n, m, order, substeps, n_mods, N, with_derivative) == (4, 2, 1, 16, 2, 6, False):
        return O.make_tdb_problem()
    return O.make_tdb_problem(N=N, n=n, m=m, order=order, seed=40 + n, substeps=substeps, n_mods=n_mods, with_derivative=with_derivative)


def _dense(r, c, j, w, wt, n_cons, n_vars):
    """J w and J' w from Jacobian values in structure order."""
    y = np.zeros(n_cons); np.add.at(y, r - 1, j * w[c - 1])
    t = np.zeros(n_vars); np.add.at(t, c - 1, j * wt[r - 1])
    return y, t


@functools.lru_cache(maxsize=None)
def case(shape):
    """Problem, point, the two vectors and the expected products: computed once, shared by every test, never written."""
    p = _problem(*shape)
    n = shape[0]
    rng = np.random.default_rng(31)
    Z = p.Z0.copy()
    if n <= 64:
        ev_o = O.OracleEvaluator(p)
        w, wt = rng.standard_normal(p.n_vars), rng.standard_normal(ev_o.n_constraints)
        ref = (ev_o.eval_constraint_jacobian_product(Z, w), ev_o.eval_constraint_jacobian_transpose_product(Z, wt))
    else:
        ev_r, _, _, j_r, _ = L.reference(p, ("products",) + tuple(shape))
        w, wt = rng.standard_normal(p.n_vars), rng.standard_normal(ev_r.n_constraints)
        r, c = ev_r.jacobian_structure1()
        ref = _dense(np.asarray(r), np.asarray(c), j_r, w, wt, ev_r.n_constraints, p.n_vars)
    for a in (Z, w, wt) + tuple(ref):
        a.setflags(write=False)
    return dict(p=p, pe=to_engine(p), Z=Z, w=w, wt=wt, Jw=ref[0], JTw=ref[1])


def _evaluator(pe, option=1, **kw):
    ev = dto_amd.Evaluator(pe, **kw)
    if option is not None:
        ev.set_option(OPTION, option)
    return ev


def check_case(shape, **kw):
    """Parity of the host and the device forms at TOL, and the two forms bit-equal."""
    check_built(case(shape), shape, **kw)


def check_built(c, shape, **kw):
    """check_case on a prepared case `c` (the keys of `case`); `shape` labels the output."""
    ev = _evaluator(c["pe"], **kw)
    try:
        yh, th = host_products(ev, c["Z"], c["w"], c["wt"])
        yd, td = dev_products(ev, c["Z"], c["w"], c["wt"])
        errs = {"Jw": rel_err(yh, c["Jw"]), "JTw": rel_err(th, c["JTw"]), "Jw_dev": rel_err(yd, c["Jw"]), "JTw_dev": rel_err(td, c["JTw"])}
        print(shape, kw, errs)
        for k, v in errs.items():
            assert v <= TOL, (shape, k, v)   # (NaN, a missing writer, fails the comparison)
        assert np.array_equal(yh, yd) and np.array_equal(th, td), shape
    finally:
        ev.close()


@pytest.mark.parametrize("shape", SCALAR)
def test_products_match_the_oracle_up_to_64_states(shape):
    check_case(shape)


@pytest.mark.parametrize("shape", MFMA)
def test_products_match_the_reference_above_64_states(shape):
    check_case(shape)


def _check_against_own_jacobian(pe, Z, **kw):
    """Products of a handle with something between the integrator's blocks against the dense products of the handle's own
    eval_constraint_jacobian values (pinned by the value tests), host and device forms."""
    ev = _evaluator(pe, **kw)
    try:
        rng = np.random.default_rng(17)
        w, wt = rng.standard_normal(ev.n_variables), rng.standard_normal(ev.n_constraints)
        j = np.full(ev.n_jacobian_entries, np.nan); ev.eval_constraint_jacobian(j, Z)
        r, c = ev.jacobian_structure()
        y_ref, t_ref = _dense(r, c, j, w, wt, ev.n_constraints, ev.n_variables)
        ev.profile_enable(); ev.profile_reset()
        yh, th = host_products(ev, Z, w, wt)
        assert ev.profile_get("tdb_product")[1] >= 2 and ev.profile_get("zero_fill")[1] == 0   # the matrix-free route, as a whole
        ev.profile_enable(False)
        yd, td = dev_products(ev, Z, w, wt)
        errs = (rel_err(yh, y_ref), rel_err(th, t_ref), rel_err(yd, y_ref), rel_err(td, t_ref))
        print("placement", errs)
        assert max(errs) <= TOL, errs
        assert np.array_equal(yh, yd) and np.array_equal(th, td)
    finally:
        ev.close()


def test_placement_at_72_states_with_a_derivative_integrator():
    p = _problem(72, 2, 1, 2, 2, 5, with_derivative=True)
    _check_against_own_jacobian(to_engine(p), p.Z0)


def test_placement_at_4_states_with_a_derivative_integrator_and_a_knot_constraint():
    p = _problem(4, 2, 1, 4, 2, 5, with_derivative=True)
    p.constraints = [O.KnotConstraint("sqnorm", [4, 5], 1.0, list(range(2, p.N + 1)), equality=False)]   # ||u||^2 - 1 <= 0
    _check_against_own_jacobian(to_engine(p), p.Z0)


def test_placement_beside_a_bilinear_integrator_on_the_same_trajectory():
    """The construction of test_time_independent_family_reproduces_the_bilinear_integrator_at_72_states with a small `substeps`
    (no agreement between the two integrators is asked for here)."""
    rng = np.random.default_rng(8)
    N, n, m = 3, 72, 1
    traj = dto_amd.NamedTrajectory({"x": rng.standard_normal((n, N)), "u": 0.3 * rng.standard_normal((m, N)),
                                    "t": np.linspace(0, 1, N)[None, :], "dt": np.full((1, N), 0.2)}, timestep="dt")
    G = 0.7 * rng.standard_normal((m + 1, n, n))
    tdb = dto_amd.TimeDependentBilinearIntegrator(dto_amd.ModulatedGenerators(G), "x", "u", "t", traj, spline_order=0, substeps=4)
    bil = dto_amd.BilinearIntegrator(G, "x", "u", traj)
    _check_against_own_jacobian(dto_amd.DirectTrajOptProblem(traj, dto_amd.NullObjective(), [tdb, bil]), traj.vec())


def _launches(ev, name):
    return ev.profile_get(name)[1]


@pytest.mark.parametrize("shape", [SCALAR[0], MFMA[1]])
def test_route(shape):
    c = case(shape)
    for option in (1, None):
        ev = _evaluator(c["pe"], option)
        try:
            ev.profile_enable(); ev.profile_reset()
            y, t = host_products(ev, c["Z"], c["w"], c["wt"])
            if option:
                assert _launches(ev, "tdb_product") >= 2
                for other in ("zero_fill", "tdb_mfma", "assembly", "jac_product"):   # (the handle has no bilinear integrator)
                    assert _launches(ev, other) == 0, other
                ms, launches, flops = ev.profile_get("tdb_product")
                ms_all, launches_all, flops_all = ev.profile_get("all")
                assert ms > 0 and flops > 0 and launches_all >= launches and flops_all >= flops
            else:
                assert _launches(ev, "tdb_product") == 0
                assert _launches(ev, "zero_fill") >= 1
            assert rel_err(y, c["Jw"]) <= TOL and rel_err(t, c["JTw"]) <= TOL
        finally:
            ev.close()


@pytest.mark.parametrize("shape", [SCALAR[3], MFMA[1]])
def test_products_repeat_bit_for_bit_and_leave_the_shared_scratch_usable(shape):
    c = case(shape)
    ev = _evaluator(c["pe"])
    try:
        Z, mu = c["Z"], c["wt"]
        Z2 = Z + 0.01 * np.random.default_rng(5).standard_normal(Z.size)

        def others(at):
            g = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(g, at)
            J = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(J, at)
            H = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(H, at, 0.7, mu)
            return g, J, H

        before = others(Z)
        runs = []
        for _ in range(3):
            runs.append(host_products(ev, Z, c["w"], c["wt"]) + dev_products(ev, Z, c["w"], c["wt"]))
            others(Z2)
        for r in runs[1:]:
            for a, b in zip(runs[0], r):
                assert np.array_equal(a, b)
        host_products(ev, Z, c["w"], c["wt"])
        for a, b in zip(before, others(Z)):
            assert np.array_equal(a, b)
    finally:
        ev.close()


@pytest.mark.parametrize("shape", [SCALAR[3], MFMA[1]])
def test_jacobian_only_handle(shape):
    check_case(shape, eval_hessian=False)


def test_both_routes_agree():
    c = case(MFMA[1])
    out = []
    for option in (0, 1):
        ev = _evaluator(c["pe"], option)
        try:
            out.append(host_products(ev, c["Z"], c["w"], c["wt"]))
        finally:
            ev.close()
    errs = (rel_err(out[1][0], out[0][0]), rel_err(out[1][1], out[0][1]))
    print("slab route against matrix-free route", errs)
    assert max(errs) <= TOL, errs
