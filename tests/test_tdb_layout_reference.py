"""CPU: the two restatements of the TimeDependentBilinearIntegrator -- `O.OracleEvaluator` (complex-step Jacobian, Richardson
differences for the Hessian) and the fast form of tests/tdb_large_cases.py (complex step throughout) -- agree on the problems of
tests/tdb_layout_cases.py: every named layout, the aliased one included, and 7 drives with the full coefficient table.  Bars are those
of tests/test_tdb_large_reference.py: 1e-10 for values and Jacobian, 1e-8 for the Hessian; structure indices bit-equal.  This is what
lets tests/test_gpu_tdb_parameters.py use `tdb_large_cases.reference` as its expected values.

Also here, on structure-only handles: what dto_create decides for these descriptions (table cap, drive count, the structured path's
keep / fall-back) and the pair-table sizes the kernels declare."""
import os
import re

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import tdb_large_cases as L
import tdb_layout_cases as C
from helpers import rel_err, to_engine


def disagreement(po, key):
    ev_o = O.OracleEvaluator(po)
    ev_f, mu, g, j, h = L.reference(po, key)
    assert np.array_equal(ev_f.jac_rows, ev_o.jac_rows) and np.array_equal(ev_f.jac_cols, ev_o.jac_cols)
    assert np.array_equal(ev_f.hess_rows, ev_o.hess_rows) and np.array_equal(ev_f.hess_cols, ev_o.hess_cols)
    Z = po.Z0
    return (rel_err(g, ev_o.eval_constraint(Z)), rel_err(j, ev_o.eval_constraint_jacobian(Z)),
            rel_err(h, ev_o.eval_hessian_lagrangian(Z, 0.6, mu)))


@pytest.mark.parametrize("layout", list(C.LAYOUTS))
def test_references_agree_on_every_layout(layout):
    """5 states, 2 drives, order 1, the mixed list [sin omega_fast, sin 0.6, cos 0, cos -1.7].

    omega_fast = 2.0 (tdb_layout_cases.OMEGA_FAST): the largest carrier, on a grid of 0.5, at which the two references agree within
    a tenth of the GPU bars (1e-11, 1e-11, 1e-9) on every problem of this file.  Values agree exactly and Jacobians to 1e-15 at any
    omega; what grows is the truncation error of the ORACLE's differenced Hessian (O(h^4 f^(6)), h = 2e-3), fastest on "t_is_dt",
    where the carrier's phase omega (1 + tau) dt_k moves through both aliased parameters.  Measured Hessian disagreement
    (default layout / t_is_dt / 7 drives / 7 drives t_is_dt):
        omega 0.0   3.7e-12  1.2e-10  2.9e-11  8.7e-11
        omega 1.0   1.1e-11  4.1e-10  2.1e-11  5.7e-11
        omega 2.0   5.7e-12  8.2e-10  5.8e-11  6.0e-10      <- chosen
        omega 2.5   1.3e-11  2.2e-09  9.5e-11  2.4e-09
        omega 4.0   1.5e-10  7.2e-09
        omega 8.0   6.4e-10  1.5e-08
        omega 12.   9.9e-09  3.9e-08
    (the fast form is a complex step of an analytic first-order sensitivity: its own error does not depend on omega)."""
    po = C.layout_problem(5, 2, 1, 4, C.MIXED, layout)
    errs = disagreement(po, ("layout-pin", layout))
    print("layout", layout, errs)
    assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-8, errs


@pytest.mark.parametrize("layout", ["default", "t_is_dt"])
def test_references_agree_at_seven_drives_with_the_full_table(layout):
    """3 states, 7 drives, order 1, four terms, N = 3: p = 16 parameters, 136 pairs.  Measured: 5.8e-11 / 6.0e-10 (Hessian)."""
    po = C.layout_problem(3, 7, 1, 2, C.MIXED, layout)
    errs = disagreement(po, ("drives-pin", layout))
    print("7 drives", layout, errs)
    assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-8, errs


def test_references_agree_without_drives():
    po = C.layout_problem(3, 0, 1, 2, C.PLAIN, "default")
    errs = disagreement(po, ("no-drives-pin",))
    assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-8, errs


def test_both_references_sum_the_aliased_parameters():
    """t_is_dt: the Jacobian column of the shared entry is the sum of the time and the timestep columns of the flow differentiated
    parameter by parameter (FastTdb._flows keeps theta = [u_k, t_k, dt_k, u_{k+1}] apart), in the oracle as in the fast form; and both
    columns are far from zero, so neither can be dropped unnoticed."""
    po = C.layout_problem(5, 2, 1, 4, C.MIXED, "t_is_dt")
    it_o, it_f = po.integrators[0], L.fast_problem(po).integrators[0]
    zz = po.Z0[:2 * po.z]
    idx, th, Phi, dPhi = it_f._flows(zz)
    m = it_f.u_dim
    assert idx[m] == idx[m + 1] == po.dt_idx
    x = zz[it_f.x_off:it_f.x_off + 5]
    col_t, col_dt = -(dPhi[m] @ x), -(dPhi[m + 1] @ x)
    assert np.abs(col_t).max() > 1e-2 and np.abs(col_dt).max() > 1e-2
    for it in (it_o, it_f):
        assert rel_err(it.jac(zz)[:, po.dt_idx], col_t + col_dt) <= 1e-12


# ---- what dto_create decides (structure-only handles: no device)

def _create(po, **kw):
    return dto_amd.Evaluator(to_engine(po), device=-1, **kw)


@pytest.mark.parametrize("n", [4, 72])
def test_the_full_table_is_accepted_and_the_next_term_is_refused(n):
    """7 drives, order 1: 153 jets x 8 generators x (1 + n_mod) -- 6120 entries at four terms, 7344 at five (cap 6144)."""
    _create(C.layout_problem(n, 7, 1, 2, C.mods_of_length(4), "default")).close()
    with pytest.raises(dto_amd.EngineError, match="coefficient table"):
        _create(C.layout_problem(n, 7, 1, 2, C.mods_of_length(5), "default")).close()


def test_order_0_takes_twelve_terms_and_not_thirteen():
    """7 drives, order 0: 55 x 8 x (1 + n_mod) -- 5720 at twelve terms, 6160 at thirteen."""
    _create(C.layout_problem(12, 7, 0, 2, C.mods_of_length(12), "default")).close()
    with pytest.raises(dto_amd.EngineError, match="coefficient table"):
        _create(C.layout_problem(12, 7, 0, 2, C.mods_of_length(13), "default")).close()


def test_eight_drives_are_refused_and_none_are_accepted():
    with pytest.raises(dto_amd.EngineError, match="0..7 drives"):
        _create(C.layout_problem(4, 8, 0, 2, (), "default")).close()
    for n in (1, 72):
        ev = _create(C.layout_problem(n, 0, 1, 2, C.PLAIN, "default"))
        assert ev.integrator_blocks(0) == (n, 1, 0)
        ev.close()


@pytest.mark.parametrize("layout,kept", [("default", 1), ("u_first", 1), ("dt_before_t", 1), ("gap", 1), ("t_is_dt", 0)])
def test_the_structured_path_keeps_disjoint_layouts_and_leaves_the_aliased_one(layout, kept):
    ev = _create(C.kron_layout_problem(12, 6, 2, 1, 2, C.MIXED[:2], layout), block_generators=True)
    try:
        assert ev.integrator_blocks(0) == (12, 6, kept)
    finally:
        ev.close()


def test_the_structured_path_takes_seven_drives_and_none():
    for m, mods in ((7, C.MIXED), (0, C.PLAIN)):
        ev = _create(C.kron_layout_problem(12, 6, m, 1, 2, mods, "default"), block_generators=True)
        try:
            assert ev.integrator_blocks(0) == (12, 6, 1)
        finally:
            ev.close()


def test_pair_tables_admit_seven_drives_at_order_1():
    """p (p + 1) / 2 = 136 at p = 16: no kernel has a pair cap below the drive cap, so there is no `largest p a kernel admits` case of
    its own -- the full-table cases of tests/test_gpu_tdb_parameters.py are the boundary."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "directtrajopt.jl_amd", "csrc")
    for name, const in (("dto_tdb_mfma.hip", "TDBM_MAX_PAIRS"), ("dto_tdb_kron.hip", "TDBK_MAX_PAIRS")):
        with open(os.path.join(src, name)) as f:
            got = re.search(r"constexpr int %s = (\d+);" % const, f.read())
        assert got and int(got.group(1)) >= 136, (name, got)
