"""CPU: the quadratic-form knot constraint g(v) = [v' M v - c] (DTO_CONSTRAINT_QUADFORM_MINUS_C) at the boundary -- the constant
in the header and both mirrors, an unchanged descriptor layout, the create-time rules, and the structure a structure-only handle
(device = -1) builds for it against the oracle's closure form of the same term."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from dto_amd import capi
from quadform_cases import check_structure, sym, with_quadforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constant_is_in_the_header_and_both_mirrors():
    header = open(os.path.join(ROOT, "include", "dto_engine.h")).read()
    assert re.search(r"#define DTO_CONSTRAINT_QUADFORM_MINUS_C 5\b", header)
    assert re.search(r"#define DTO_ABI_VERSION 8\b", header)
    assert capi.CONSTRAINT_QUADFORM == 5 and capi.DTO_ABI_VERSION == 8
    assert dto_amd.NonlinearKnotPointConstraint.KINDS["quadform"] == 5
    shim = open(os.path.join(ROOT, "integration", "DTOEngine.jl")).read()
    assert re.search(r"const DTO_CONSTRAINT_QUADFORM_MINUS_C = Int32\(5\)", shim)
    assert "DTO_CONSTRAINT_QUADFORM_MINUS_C," in shim  # the descriptor builder emits the kind


def test_the_descriptor_keeps_its_layout():
    assert C.sizeof(capi.ConstraintDesc) == 64
    assert capi.ConstraintDesc.hess0.offset == 56 and capi.ConstraintDesc.jac0.offset == 48


def _create(kind=5, n=3, M="sym", comps=(0, 1, 2), times=(2, 4), N=5, z=6):
    """dto_create on a structure-only description with one derivative integrator and one constraint; (rc, error text)."""
    lib = dto_amd.load_library()
    rng = np.random.default_rng(0)
    integ = (capi.IntegratorDesc * 1)(capi.IntegratorDesc(capi.INTEGRATOR_DERIVATIVE, 0, 2, 2, 2, None))
    comps = np.ascontiguousarray(comps, dtype=np.int32)
    t = np.ascontiguousarray(times, dtype=np.int64)
    Mm = None if M is None else (np.ascontiguousarray(sym(rng, n)) if isinstance(M, str) else np.ascontiguousarray(M, dtype=np.float64))
    cons = (capi.ConstraintDesc * 1)(capi.ConstraintDesc(kind, 0, comps.size, 1, comps.ctypes.data_as(capi.c_int32_p), 0.5,
                                                          t.ctypes.data_as(capi.c_int64_p), t.size, None,
                                                          None if Mm is None else Mm.ctypes.data_as(capi.c_double_p)))
    objs = (capi.ObjectiveDesc * 1)()
    Z0 = np.ascontiguousarray(rng.standard_normal(z * N))
    desc = capi.ProblemDesc(capi.DTO_ABI_VERSION, -1, N, z, 0, z - 1, 1, 1, 0, 1, 0, integ, objs, cons,
                            Z0.ctypes.data_as(capi.c_double_p), 0, 0)
    h = capi.H()
    rc = lib.dto_create(C.byref(desc), C.byref(h))
    text = "" if rc == 0 else lib.dto_last_error(None).decode()
    if rc == 0:
        n_cons = C.c_int64()
        lib.dto_num_cons(h, C.byref(n_cons))
        assert n_cons.value == 2 * (N - 1) + len(times)
        lib.dto_destroy(h)
    return rc, text


def test_create_accepts_a_valid_description():
    assert _create() == (0, "")


def test_create_refuses_a_missing_matrix():
    rc, text = _create(M=None)
    assert rc != 0 and "hess0" in text


def test_create_refuses_an_asymmetric_matrix():
    M = np.eye(3)
    M[0, 2] = 1e-300
    rc, text = _create(M=M)
    assert rc != 0 and "symmetric" in text


def test_create_refuses_a_component_listed_twice():
    rc, text = _create(comps=(0, 1, 0))
    assert rc != 0 and "twice" in text


@pytest.mark.parametrize("times", [(0, 2), (2, 6)])
def test_create_refuses_times_outside_the_horizon(times):
    rc, text = _create(times=times)
    assert rc != 0 and "time" in text


def test_the_python_mirror_checks_the_matrix():
    pe = dto_amd.synthetic.make_scaled_problem(4, 3, 2)
    with pytest.raises(ValueError):
        dto_amd.NonlinearKnotPointConstraint("quadform", "x", pe.trajectory)
    with pytest.raises(ValueError):
        dto_amd.NonlinearKnotPointConstraint("quadform", "x", pe.trajectory, M=np.triu(np.ones((3, 3))))
    con = dto_amd.fidelity_constraint(np.ones((2, 3)), "x", pe.trajectory, 0.9)
    assert con.kind == "quadform" and con.c == -0.9 and not con.equality and list(con.times) == [4]
    assert np.array_equal(con.M, np.full((3, 3), -2.0))  # -A'A


def _structure_case(specs, N=6, n=5, m=2, seed=3, zero_knot=None):
    base = O.make_scaled_problem(N, n, m, seed=seed, with_constraint=True)
    if zero_knot is not None:
        base.Z0.reshape(N, base.z)[zero_knot - 1, :n] = 0.0
    prob_o, prob_e, _ = with_quadforms(base, specs)
    ev_o = O.OracleEvaluator(prob_o)
    ev = dto_amd.Evaluator(prob_e, device=-1)
    try:
        assert ev.n_constraints == ev_o.n_constraints and ev.n_variables == prob_o.n_vars
        check_structure(ev, ev_o)
        return ev.jacobian_structure(), ev_o
    finally:
        ev.close()


def test_structure_and_bounds_for_a_random_symmetric_matrix():
    rng = np.random.default_rng(1)
    _structure_case([dict(comps=[0, 1, 2, 3, 4], times1=[1, 3, 6], M=sym(rng, 5), c=0.3, equality=False),
                     dict(comps=[6, 2, 0], times1=[2, 2, 5], M=sym(rng, 3), c=-1.0, equality=True)])


def test_columns_of_structurally_zero_rows_are_absent():
    rng = np.random.default_rng(2)
    M = sym(rng, 5)
    M[[1, 3], :] = 0.0
    M[:, [1, 3]] = 0.0
    (rows, cols), ev_o = _structure_case([dict(comps=[0, 1, 2, 3, 4], times1=[2, 4], M=M, c=0.0, equality=False)], N=6, n=5, m=2)
    z = 5 + 2 * 2 + 1
    first_row = ev_o.n_dynamics_constraints + 4 + 1  # behind the base problem's four norm rows (times 2..5), 1-based
    mine = cols[rows >= first_row]
    assert sorted(mine.tolist()) == sorted([(t - 1) * z + c + 1 for t in (2, 4) for c in (0, 2, 4)])


def test_a_listed_knot_with_a_zero_state_has_no_entries():
    rng = np.random.default_rng(4)
    (rows, cols), ev_o = _structure_case([dict(comps=[0, 1, 2, 3, 4], times1=[2, 3], M=sym(rng, 5), c=1.0, equality=False)],
                                         zero_knot=3)
    first_row = ev_o.n_dynamics_constraints + 4 + 1
    assert np.count_nonzero(rows == first_row) == 5 and np.count_nonzero(rows == first_row + 1) == 0
