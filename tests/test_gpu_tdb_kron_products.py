"""GPU: matrix-free J w / J' w on the structured time-dependent path (option "tdb_matrix_free_products" = 1 on a handle whose
TimeDependentBilinearIntegrator has replicated-block generators; k_tdb_kron_product in csrc/dto_tdb_kron.hip).

Expected values never come from the engine: the oracle evaluator's Jacobian values of the problem with the integrator in the fast
form of tests/tdb_large_cases.py (the Jacobian alone, no Hessian), contracted with np.add.at.  The bar is helpers.TOL,
1e-10 max(1, |ref|), the project's bar for first-order quantities.  Outputs are filled with NaN beforehand so that a missing
writer shows.  Cases are (b, r, m, order, substeps, n_mods), N = 3 unless stated."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import tdb_large_cases as L
from helpers import TOL, rel_err, to_engine
from tdb_block_cases import kron_family, kron_tdb_problem
from test_gpu_jacobian_products import dev_products, host_products
from test_gpu_tdb_block_generators import CASES as VALUE_CASES, _to_oracle
from test_gpu_tdb_products import _check_against_own_jacobian, _dense

pytestmark = pytest.mark.gpu

OPTION = "tdb_matrix_free_products"
# MT 1..4, padded and ragged blocks, the 64-row cap and 512 states; four finest blocks grouped into a 16-row working block; three
# grouped, 15 of 16 rows; cp = 32, two column tiles per group
CASES = list(VALUE_CASES) + [(4, 16, 1, 0, 2, 1), (5, 9, 1, 0, 2, 1), (16, 20, 1, 0, 2, 1)]


@functools.lru_cache(maxsize=None)
def case(shape, N=3):
    """Problem, point, the two vectors and the expected products: computed once, shared by every test, never written."""
    po = kron_tdb_problem(*shape, N=N)
    ev_o = O.OracleEvaluator(L.fast_problem(po))
    rng = np.random.default_rng(31)
    Z = po.Z0.copy()
    w, wt = rng.standard_normal(po.n_vars), rng.standard_normal(ev_o.n_constraints)
    r, c = ev_o.jacobian_structure1()
    ref = _dense(np.asarray(r), np.asarray(c), ev_o.eval_constraint_jacobian(Z), w, wt, ev_o.n_constraints, po.n_vars)
    for a in (Z, w, wt) + tuple(ref):
        a.setflags(write=False)
    return dict(po=po, pe=to_engine(po), Z=Z, w=w, wt=wt, Jw=ref[0], JTw=ref[1])


def _evaluator(pe, option=1, **kw):
    ev = dto_amd.Evaluator(pe, block_generators=True, **kw)
    if option is not None:
        ev.set_option(OPTION, option)
    return ev


def _launches(ev, name):
    return ev.profile_get(name)[1]


def _check(shape, **kw):
    """Parity of the host and device forms with the oracle at TOL, the two forms bit-equal, and the route by its launches."""
    c = case(shape)
    ev = _evaluator(c["pe"], **kw)
    try:
        assert ev.integrator_blocks(0)[2] == 1, ev.integrator_blocks(0)
        ev.profile_enable(); ev.profile_reset()
        yh, th = host_products(ev, c["Z"], c["w"], c["wt"])
        counts = {k: _launches(ev, k) for k in ("tdb_product", "tdb_kron", "tdb_mfma", "zero_fill")}
        ev.profile_enable(False)
        yd, td = dev_products(ev, c["Z"], c["w"], c["wt"])
        errs = {"Jw": rel_err(yh, c["Jw"]), "JTw": rel_err(th, c["JTw"]), "Jw_dev": rel_err(yd, c["Jw"]), "JTw_dev": rel_err(td, c["JTw"])}
        print(shape, kw, ev.integrator_blocks(0), errs, counts)
        for k, v in errs.items():
            assert v <= TOL, (shape, k, v)   # (NaN, a missing writer, fails the comparison)
        assert np.array_equal(yh, yd) and np.array_equal(th, td), shape
        assert counts == {"tdb_product": 2, "tdb_kron": 0, "tdb_mfma": 0, "zero_fill": 0}, (shape, counts)
    finally:
        ev.close()


@pytest.mark.parametrize("shape", CASES)
def test_products_match_the_oracle_on_the_matrix_free_route(shape):
    _check(shape)


def test_default_option_keeps_the_slab_route_and_both_routes_agree():
    c = case(VALUE_CASES[1])
    out = []
    for option in (None, 0, 1):
        ev = _evaluator(c["pe"], option)
        try:
            ev.profile_enable(); ev.profile_reset()
            out.append(host_products(ev, c["Z"], c["w"], c["wt"]))
            if not option:
                assert _launches(ev, "tdb_product") == 0 and _launches(ev, "tdb_kron") >= 1
        finally:
            ev.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    errs = (rel_err(out[2][0], out[1][0]), rel_err(out[2][1], out[1][1]), rel_err(out[1][0], c["Jw"]), rel_err(out[1][1], c["JTw"]))
    print("matrix-free route against slab route, slab route against the oracle", errs)
    assert max(errs) <= TOL, errs


def test_products_do_not_depend_on_the_persistent_grid():
    """Seven intervals on grids of 3, 1 and the default: a workgroup walks several intervals through one scratch slot."""
    c = case((12, 6, 2, 1, 2, 2), N=8)
    ev = _evaluator(c["pe"])
    try:
        runs = []
        for resident in (3, 1, 0):
            ev.set_option("tdb_resident", resident)
            runs.append(host_products(ev, c["Z"], c["w"], c["wt"]) + dev_products(ev, c["Z"], c["w"], c["wt"]))
        errs = (rel_err(runs[0][0], c["Jw"]), rel_err(runs[0][1], c["JTw"]))
        print("persistent grid", errs)
        assert max(errs) <= TOL, errs
        for r in runs[1:]:
            for a, b in zip(runs[0], r):
                assert np.array_equal(a, b)
    finally:
        ev.close()


def test_placement_with_a_derivative_integrator_between_the_blocks():
    po = kron_tdb_problem(12, 6, 2, 1, 2, 2, N=5, with_derivative=True)
    _check_against_own_jacobian(to_engine(po), po.Z0, block_generators=True)


def test_unitary_tdb_problem_products_match_the_oracle():
    pe = dto_amd.synthetic.unitary_tdb_problem(levels=6, drives=2, N=4)
    po = _to_oracle(pe)
    ev_o = O.OracleEvaluator(L.fast_problem(po))
    rng = np.random.default_rng(9)
    w, wt = rng.standard_normal(po.n_vars), rng.standard_normal(ev_o.n_constraints)
    y_ref, t_ref = ev_o.eval_constraint_jacobian_product(po.Z0, w), ev_o.eval_constraint_jacobian_transpose_product(po.Z0, wt)
    ev = _evaluator(pe)
    try:
        assert ev.integrator_blocks(0) == (12, 6, 1)
        ev.profile_enable(); ev.profile_reset()
        yh, th = host_products(ev, po.Z0, w, wt)
        assert _launches(ev, "tdb_product") == 2 and _launches(ev, "tdb_kron") == 0 and _launches(ev, "zero_fill") == 0
        ev.profile_enable(False)
        yd, td = dev_products(ev, po.Z0, w, wt)
        errs = (rel_err(yh, y_ref), rel_err(th, t_ref), rel_err(yd, y_ref), rel_err(td, t_ref))
        print("unitary tdb products", errs)
        assert max(errs) <= TOL, errs
        assert np.array_equal(yh, yd) and np.array_equal(th, td)
    finally:
        ev.close()


def test_structured_and_dense_integrators_of_one_handle_go_matrix_free_together():
    """A 12 x 6 structured integrator and a 4-state dense one (k_tdb) on one trajectory, sharing controls and time."""
    rng = np.random.default_rng(12)
    N, m = 4, 2
    G, mods = kron_family(12, 6, m, 2, rng)
    traj = dto_amd.NamedTrajectory({"x": rng.standard_normal((72, N)), "y": rng.standard_normal((4, N)), "u": 0.4 * rng.standard_normal((m, N)),
                                    "t": np.cumsum(np.full(N, 0.3))[None, :], "dt": 0.25 + 0.1 * rng.random((1, N))}, timestep="dt")
    big = dto_amd.TimeDependentBilinearIntegrator(dto_amd.ModulatedGenerators(G, mods), "x", "u", "t", traj, spline_order=1, substeps=2)
    Gs = 0.7 * rng.standard_normal((m + 1, 4, 4))
    small = dto_amd.TimeDependentBilinearIntegrator(dto_amd.ModulatedGenerators(Gs, [("cos", 1.1, 0.3 * rng.standard_normal((m + 1, 4, 4)))]),
                                                    "y", "u", "t", traj, spline_order=1, substeps=3)
    pe = dto_amd.DirectTrajOptProblem(traj, dto_amd.NullObjective(), [big, small])
    probe = dto_amd.Evaluator(pe, block_generators=True)
    try:
        assert probe.integrator_blocks(0) == (12, 6, 1) and probe.integrator_blocks(1)[2] == 0
    finally:
        probe.close()
    _check_against_own_jacobian(pe, traj.vec(), block_generators=True)
    ev = _evaluator(pe)
    try:
        w, wt = rng.standard_normal(ev.n_variables), rng.standard_normal(ev.n_constraints)
        ev.profile_enable(); ev.profile_reset()
        host_products(ev, traj.vec(), w, wt)
        assert _launches(ev, "tdb_product") == 4 and _launches(ev, "tdb_kron") == 0 and _launches(ev, "zero_fill") == 0
    finally:
        ev.close()


def test_products_repeat_bit_for_bit_and_leave_the_shared_scratch_usable():
    c = case(VALUE_CASES[1])
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


def test_jacobian_only_handle():
    _check((12, 6, 2, 1, 4, 2), eval_hessian=False)
