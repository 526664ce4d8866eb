"""GPU: Hessian-of-Lagrangian-vector products y = H(Z; sigma, mu) v (dto_eval_hessian_product[_dev],
MOI.eval_hessian_lagrangian_product) against the oracle, against the engine's own Hessian, and their point cache.

The reference product is the oracle's Hessian values on its 1-based structure as a sparse matrix with duplicates summed,
H v + H' v - diag(H) v (the slab holds the upper triangle; MOI counts an off-diagonal entry for (i, j) and (j, i)).  Bar:
1e-8 max(1, |ref|), the Hessian's.  Every oracle case also asserts the path it ran through the profile counters."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import dto_oracle as O
from helpers import rel_err, to_engine

pytestmark = pytest.mark.gpu

TOL_H = 1e-8


def _sym_product(rows1, cols1, vals, v):
    n = v.size
    H = sp.coo_matrix((vals, (np.asarray(rows1) - 1, np.asarray(cols1) - 1)), shape=(n, n)).tocsr()  # duplicates summed
    return H @ v + H.T @ v - H.diagonal() * v


def _oracle_product(ev_o, Z, sigma, mu, v):
    r1, c1 = ev_o.hessian_structure1()
    return _sym_product(r1, c1, ev_o.eval_hessian_lagrangian(Z, sigma, mu), v)


def _product(ev, Z, v, sigma, mu):
    y = np.full(ev.n_variables, np.nan)
    ev.eval_hessian_lagrangian_product(y, Z, v, sigma, mu)
    return y


def _launches(ev, name):
    return ev.profile_get(name)[1]


def _large_norm_point(p):
    rng = np.random.default_rng(1)
    Z = p.Z0 + 0.3 * rng.standard_normal(p.n_vars)
    Z[p.dt_idx::p.z] = 0.9 + 0.2 * rng.random(p.N)  # big steps: several squarings, q > 1 (test_gpu_parity)
    return Z


# (problem, closure derivatives, point, path): "small" = the one-workgroup path (n <= 32, no profiled sweep launch), "sweep" =
# the Hessian's adjoint sweep ran, "host" = no bilinear integrator / host-merged blocks only (no sweep)
CASES = {
    "readme": (lambda: O.make_readme_problem(), "numeric", None, "small"),
    "standard": (lambda: O.make_standard_problem(N=10), "numeric", None, "small"),
    "n3": (lambda: O.make_scaled_problem(5, 3, 2, seed=3, with_constraint=True), "numeric", None, "small"),
    "n17": (lambda: O.make_scaled_problem(5, 17, 3, seed=17, with_constraint=True), "numeric", None, "small"),
    "n32": (lambda: O.make_scaled_problem(5, 32, 2, seed=32, with_constraint=True), "numeric", None, "small"),
    "n64": (lambda: O.make_scaled_problem(5, 64, 4, seed=64, with_constraint=True), "numeric", None, "sweep"),
    "n70": (lambda: O.make_scaled_problem(4, 70, 2, seed=70, with_constraint=True), "numeric", None, "sweep"),
    "n128": (lambda: O.make_scaled_problem(4, 128, 2, seed=128, with_constraint=True), "numeric", None, "sweep"),
    "n256": (lambda: O.make_scaled_problem(3, 256, 2, seed=256, with_constraint=True), "numeric", None, "sweep"),
    "n300": (lambda: O.make_scaled_problem(3, 300, 1, seed=300, with_constraint=True), "numeric", None, "sweep"),
    "large-norm": (lambda: O.make_scaled_problem(5, 16, 2, seed=11, with_constraint=True), "numeric", _large_norm_point, "small"),
    "closure": (lambda: O.make_closure_problem(), "analytic", None, "any"),
    "global": (lambda: O.make_global_problem(), "analytic", None, "any"),
    "external-integrator": (lambda: O.make_external_integrator_problem(), "analytic", None, "any"),
    "tdb": (lambda: O.make_tdb_problem(), "numeric", None, "any"),
    "ket": (lambda: O.make_ket_problem(), "numeric", None, "any"),
    "l1-slack-1024": (lambda: O.make_l1_slack_problem(3, 1024, 4), "numeric", None, "sweep"),
    "type1-derivative": (lambda: O.make_type1_derivative_problem(), "numeric", None, "any"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_product_matches_the_oracle(case):
    import dto_amd
    make, deriv, point, path = CASES[case]
    p = make()
    ev_o = O.OracleEvaluator(p)
    ev = dto_amd.Evaluator(to_engine(p, deriv))
    try:
        rng = np.random.default_rng(7)
        Z = p.Z0.copy() if point is None else point(p)
        mu = rng.standard_normal(ev.n_constraints)
        v = rng.standard_normal(ev.n_variables)
        sigma = 0.7
        ev.profile_enable(True)
        ev.profile_reset()
        y = _product(ev, Z, v, sigma, mu)
        counts = {k: _launches(ev, k) for k in ("expmv", "expmv_adjoint", "hess_product", "zero_fill")}
        stats = ev.last_stats()
        ref = _oracle_product(ev_o, Z, sigma, mu, v)
        err = rel_err(y, ref)
        print(case, err, counts, stats)
        assert np.all(np.isfinite(y)) and err <= TOL_H, (case, err)
        assert counts["hess_product"] == 2, counts  # the gather into the compact copy, then the product
        if path == "small":
            assert counts["expmv_adjoint"] == 0 and counts["expmv"] == 0, counts
        elif path == "sweep":
            assert counts["expmv_adjoint"] >= 1, counts
        # sigma = 0: the objective's terms drop out as in eval_hessian_lagrangian
        y0 = _product(ev, Z, v, 0.0, mu)
        assert rel_err(y0, _oracle_product(ev_o, Z, 0.0, mu, v)) <= TOL_H
    finally:
        ev.close()


def test_product_matches_the_engines_own_hessian_and_the_device_form():
    """256 x 200: the product equals numpy's symmetric product of what eval_hessian_lagrangian returns at the same point (to the
    summation order), and the device-pointer form returns the host form's bits."""
    import dto_amd
    import torch
    p = O.make_scaled_problem(200, 256, 2, seed=4, with_constraint=True)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        rng = np.random.default_rng(2)
        Z = p.Z0 + 0.01 * rng.standard_normal(p.n_vars)
        mu = rng.standard_normal(ev.n_constraints)
        v = rng.standard_normal(ev.n_variables)
        y = _product(ev, Z, v, 0.7, mu)
        h = np.empty(ev.n_hessian_entries); ev.eval_hessian_lagrangian(h, Z, 0.7, mu)
        r, c = ev.hessian_lagrangian_structure()
        ref = _sym_product(r, c, h, v)
        del h, r, c
        assert rel_err(y, ref) <= 1e-13, rel_err(y, ref)
        dev = torch.device("cuda:0")
        st = torch.cuda.current_stream(dev).cuda_stream
        dZ, dmu, dv = (torch.from_numpy(a).to(dev) for a in (Z, mu, v))
        dy = torch.full((ev.n_variables,), float("nan"), dtype=torch.float64, device=dev)
        ev2 = dto_amd.Evaluator(to_engine(p))  # a fresh handle: the device form assembles its own Hessian
        try:
            ev2.eval_hessian_product_dev(dZ.data_ptr(), 0.7, dmu.data_ptr(), dv.data_ptr(), dy.data_ptr(), st)
            torch.cuda.synchronize()
            assert np.array_equal(dy.cpu().numpy(), y)
            dy.fill_(float("nan"))
            ev.eval_hessian_product_dev(dZ.data_ptr(), 0.7, dmu.data_ptr(), dv.data_ptr(), dy.data_ptr(), st)  # cached point
            torch.cuda.synchronize()
            assert np.array_equal(dy.cpu().numpy(), y)
        finally:
            ev2.close()
    finally:
        ev.close()


def test_symmetry_and_linearity():
    import dto_amd
    p = O.make_scaled_problem(6, 40, 3, seed=9, with_constraint=True)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        rng = np.random.default_rng(4)
        Z = p.Z0 + 0.02 * rng.standard_normal(p.n_vars)
        mu = rng.standard_normal(ev.n_constraints)
        u, v, w = (rng.standard_normal(ev.n_variables) for _ in range(3))
        Hu, Hv, Hw = (_product(ev, Z, x, 0.7, mu) for x in (u, v, w))
        a, b = u @ Hv, v @ Hu
        assert abs(a - b) <= 1e-12 * max(1.0, abs(a)), (a, b)
        al, be = 0.37, -1.9
        Hc = _product(ev, Z, al * v + be * w, 0.7, mu)
        assert rel_err(Hc, al * Hv + be * Hw) <= 1e-12
    finally:
        ev.close()


def test_second_product_at_the_same_point_is_one_launch():
    import dto_amd
    p = O.make_scaled_problem(4, 256, 2, seed=8, with_constraint=True)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        rng = np.random.default_rng(5)
        Z = p.Z0.copy()
        mu = rng.standard_normal(ev.n_constraints)
        ev.profile_enable(True)
        ev.profile_reset()
        y1 = _product(ev, Z, rng.standard_normal(ev.n_variables), 0.7, mu)
        names = ("all", "hess_product", "expmv", "expmv_adjoint", "zero_fill")
        before = {k: _launches(ev, k) for k in names}
        assert before["expmv_adjoint"] >= 1 and before["hess_product"] == 2, before
        v2 = rng.standard_normal(ev.n_variables)
        y2 = _product(ev, Z, v2, 0.7, mu)
        after = {k: _launches(ev, k) for k in names}
        grew = after["hess_product"] - before["hess_product"]
        assert grew >= 1 and after["all"] - before["all"] == grew, (before, after)
        for k in ("expmv", "expmv_adjoint", "zero_fill"):
            assert after[k] == before[k], (k, before, after)
        assert not np.array_equal(y1, y2)
        ev_o = O.OracleEvaluator(p)
        assert rel_err(y2, _oracle_product(ev_o, Z, 0.7, mu, v2)) <= TOL_H
    finally:
        ev.close()


def test_one_ulp_changes_start_a_new_point():
    """A product after a one-ulp change of Z alone, of sigma alone or of mu alone assembles anew (launch counts) and returns a
    fresh handle's bits for that point."""
    import dto_amd
    p = O.make_scaled_problem(6, 40, 3, seed=12, with_constraint=True)
    rng = np.random.default_rng(6)
    Z = p.Z0 + 0.02 * rng.standard_normal(p.n_vars)
    mu = rng.standard_normal(O.OracleEvaluator(p).n_constraints)
    v = rng.standard_normal(p.n_vars)
    Z1 = Z.copy(); Z1[p.z + 1] = np.nextafter(Z1[p.z + 1], np.inf)
    mu1 = mu.copy(); mu1[3] = np.nextafter(mu1[3], -np.inf)
    s1 = np.nextafter(0.7, 1.0)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        ev.profile_enable(True)
        ev.profile_reset()
        _product(ev, Z, v, 0.7, mu)
        for Zc, sc, mc in ((Z1, 0.7, mu), (Z, s1, mu), (Z, 0.7, mu1)):
            _product(ev, Z, v, 0.7, mu)  # back at the cached point
            n0 = _launches(ev, "hess_product")
            y = _product(ev, Zc, v, sc, mc)
            assert _launches(ev, "hess_product") - n0 == 2  # gather + product: the Hessian was assembled again
            fresh = dto_amd.Evaluator(to_engine(p))
            try:
                assert np.array_equal(y, _product(fresh, Zc, v, sc, mc))
            finally:
                fresh.close()
    finally:
        ev.close()


def _raw_hessian_product(ev, Z, sigma, mu, v):
    """The engine's Hessian at (Z, sigma, mu) with whatever external blocks are staged, multiplied by numpy."""
    h = np.empty(ev.n_hessian_entries)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert ev._lib.dto_eval_hessian(ev.handle, dp(Z), sigma, dp(mu), dp(h)) == 0, ev._lib.dto_last_error(ev.handle)
    r, c = ev.hessian_lagrangian_structure()
    return _sym_product(r, c, h, v)


def test_new_external_blocks_at_the_same_point_take_effect():
    import dto_amd
    p = O.make_closure_problem()
    ev = dto_amd.Evaluator(to_engine(p, "analytic"))
    ref = dto_amd.Evaluator(to_engine(p, "analytic"))
    try:
        rng = np.random.default_rng(8)
        Z = p.Z0.copy()
        Z2 = p.Z0 + 0.05 * rng.standard_normal(p.n_vars)
        mu = rng.standard_normal(ev.n_constraints)
        v = rng.standard_normal(ev.n_variables)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        y1 = _product(ev, Z, v, 0.7, mu)
        assert rel_err(y1, _oracle_product(O.OracleEvaluator(p), Z, 0.7, mu, v)) <= TOL_H
        # the closure blocks of another point, the built-in terms at Z
        ev._stage_external(Z2, con_need=2, obj_need=2, mu=mu)
        y2 = np.full(ev.n_variables, np.nan)
        assert ev._lib.dto_eval_hessian_product(ev.handle, dp(Z), 0.7, dp(mu), dp(v), dp(y2)) == 0
        ref._stage_external(Z2, con_need=2, obj_need=2, mu=mu)
        want = _raw_hessian_product(ref, Z, 0.7, mu, v)
        assert not np.array_equal(y1, y2)
        assert rel_err(y2, want) <= 1e-13, rel_err(y2, want)
    finally:
        ev.close()
        ref.close()


def test_interleaved_callbacks_leave_every_result_correct():
    """eval_hessian, eval_jacobian and a bound device Hessian between products on one handle."""
    import dto_amd
    import torch
    p = O.make_scaled_problem(5, 128, 2, seed=14, with_constraint=True)
    ev_o = O.OracleEvaluator(p)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        rng = np.random.default_rng(9)
        Z1, Z2 = p.Z0.copy(), p.Z0 + 0.02 * rng.standard_normal(p.n_vars)
        mu1, mu2 = rng.standard_normal(ev.n_constraints), rng.standard_normal(ev.n_constraints)
        v = rng.standard_normal(ev.n_variables)
        dev = torch.device("cuda:0")
        st = torch.cuda.current_stream(dev).cuda_stream
        bound = torch.full((ev.n_hessian_entries,), float("nan"), dtype=torch.float64, device=dev)
        ev.bind_output_dev(2, bound.data_ptr())
        ref1, ref2 = _oracle_product(ev_o, Z1, 0.7, mu1, v), _oracle_product(ev_o, Z2, 0.7, mu2, v)
        hess_ref2 = ev_o.eval_hessian_lagrangian(Z2, 0.7, mu2)
        y1 = _product(ev, Z1, v, 0.7, mu1)
        assert rel_err(y1, ref1) <= TOL_H
        h = np.empty(ev.n_hessian_entries); ev.eval_hessian_lagrangian(h, Z2, 0.7, mu2)
        assert rel_err(h, hess_ref2) <= TOL_H
        assert np.array_equal(_product(ev, Z1, v, 0.7, mu1), y1)
        j = np.empty(ev.n_jacobian_entries); ev.eval_constraint_jacobian(j, Z2)
        assert rel_err(j, ev_o.eval_constraint_jacobian(Z2)) <= 1e-10
        dZ2, dmu2 = torch.from_numpy(Z2).to(dev), torch.from_numpy(mu2).to(dev)
        for _ in range(2):  # the second call into the bound vector writes only what can change
            ev.eval_hessian_dev(dZ2.data_ptr(), 0.7, dmu2.data_ptr(), bound.data_ptr(), st)
            torch.cuda.synchronize()
            assert rel_err(bound.cpu().numpy(), hess_ref2) <= TOL_H
            y2 = _product(ev, Z2, v, 0.7, mu2)
            assert rel_err(y2, ref2) <= TOL_H
            assert np.array_equal(_product(ev, Z1, v, 0.7, mu1), y1)
        ev.eval_hessian_dev(dZ2.data_ptr(), 0.7, dmu2.data_ptr(), bound.data_ptr(), st)
        torch.cuda.synchronize()
        assert rel_err(bound.cpu().numpy(), hess_ref2) <= TOL_H
    finally:
        ev.close()


def test_repeated_products_return_the_same_bits():
    """Ten repeats under default options, each at a point the handle has to assemble again (another point in between)."""
    import dto_amd
    p = O.make_scaled_problem(40, 130, 2, seed=2, with_constraint=True)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        rng = np.random.default_rng(10)
        Z = p.Z0 + 0.01 * rng.standard_normal(p.n_vars)
        mu = rng.standard_normal(ev.n_constraints)
        v = rng.standard_normal(ev.n_variables)
        first = _product(ev, Z, v, 0.7, mu)
        for rep in range(10):
            _product(ev, Z + 0.01 * rep, v, 0.7, mu)
            assert np.array_equal(_product(ev, Z, v, 0.7, mu), first), rep
            assert np.array_equal(_product(ev, Z, v, 0.7, mu), first), rep  # the cached point
    finally:
        ev.close()


def test_handles_without_the_product_return_errors():
    import dto_amd
    p = O.make_scaled_problem(6, 8, 2, seed=2, with_constraint=True)
    rng = np.random.default_rng(11)
    v = rng.standard_normal(p.n_vars)
    ev = dto_amd.Evaluator(to_engine(p), eval_hessian=False)
    try:
        with pytest.raises(dto_amd.EngineError, match="eval_hessian = 0"):
            _product(ev, p.Z0, v, 1.0, np.zeros(ev.n_constraints))
    finally:
        ev.close()
    ev = dto_amd.Evaluator(to_engine(p), k_lo=2, k_hi=p.N)
    try:
        with pytest.raises(dto_amd.EngineError, match="unsharded"):
            _product(ev, p.Z0, v, 1.0, np.zeros(ev.n_constraints))
        # the handle still evaluates afterwards
        h = np.empty(ev.shard.hess_len); ev.eval_hessian_lagrangian(h, p.Z0, 1.0, np.zeros(ev.n_constraints))
    finally:
        ev.close()
