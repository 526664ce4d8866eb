"""CPU: dto_dynamics_layout / dto_dynamics_solve_all / dto_dynamics_solve_all_dev at the boundary -- exported by the built library,
typed alike in the header, ctypes and the Julia binding, the header's declared set equal to capi.SYMBOLS, ABI version still 8, no name
with `tdb` in it, and a structure-only handle (no device) answers the layout, refuses the solves with text and stays usable."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from elim_cases import REFUSED_LAYOUTS, RawDerivativeHandle, describe, plan, three_level_problem
from helpers import to_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = open(os.path.join(ROOT, "include", "dto_engine.h"), encoding="utf-8").read()
H_NOCOMMENT = re.sub(r"/\*.*?\*/", "", H, flags=re.S)
JL = open(os.path.join(ROOT, "integration", "DTOEngine.jl"), encoding="utf-8").read()
NAMES = ("dto_dynamics_layout", "dto_dynamics_solve_all", "dto_dynamics_solve_all_dev")

LAYOUT_ARGS = ["const dto_handle* h", "int32_t* n_states", "int32_t* n_levels", "int32_t* offset", "int32_t* level"]
HOST_ARGS = ["dto_handle* h", "const double* Z", "int32_t direction", "const double* B", "int32_t n_cols", "double* Y"]
DEV_ARGS = ["dto_handle* h", "const double* dZ", "int32_t direction", "const double* dB", "int32_t n_cols", "double* dY", "void* stream"]


def _c_args(name):
    m = re.search(r"^int\s+%s\((.*?)\);" % name, H_NOCOMMENT, flags=re.S | re.M)
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def _jl_args(name):
    m = re.search(r"@ccall\(?\s*lib\.%s\((.*?)\)::(\w+)" % name, JL, flags=re.S)
    assert m and m.group(2) == "Cint", name
    return [a.split("::")[-1].strip() for a in re.split(r",(?![^{]*\})", m.group(1))]


def test_the_symbols_are_exported_by_the_built_library():
    lib = dto_amd.load_library()
    for name in NAMES:
        assert name in dto_amd.capi.SYMBOLS and hasattr(lib, name), name


def test_typed_alike_in_header_ctypes_and_julia():
    H_, dp, ip = dto_amd.capi.H, dto_amd.capi.c_double_p, dto_amd.capi.c_int32_p
    assert _c_args("dto_dynamics_layout") == LAYOUT_ARGS
    assert _c_args("dto_dynamics_solve_all") == HOST_ARGS
    assert _c_args("dto_dynamics_solve_all_dev") == DEV_ARGS
    res, args = dto_amd.capi.SYMBOLS["dto_dynamics_layout"]
    assert res is C.c_int and list(args) == [H_, ip, ip, ip, ip]
    res, args = dto_amd.capi.SYMBOLS["dto_dynamics_solve_all"]
    assert res is C.c_int and list(args) == [H_, dp, C.c_int32, dp, C.c_int32, dp]
    res, args = dto_amd.capi.SYMBOLS["dto_dynamics_solve_all_dev"]
    assert res is C.c_int and list(args) == [H_, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    assert _jl_args("dto_dynamics_layout") == ["Ptr{Cvoid}", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Int32}"]
    assert _jl_args("dto_dynamics_solve_all") == ["Ptr{Cvoid}", "Ptr{Float64}", "Int32", "Ptr{Float64}", "Int32", "Ptr{Float64}"]
    assert _jl_args("dto_dynamics_solve_all_dev") == ["Ptr{Cvoid}", "Ptr{Float64}", "Int32", "Ptr{Float64}", "Int32", "Ptr{Float64}", "Ptr{Cvoid}"]
    for fn in ("dynamics_layout", "dynamics_solve_all", r"dynamics_solve_all_dev!"):
        assert re.search(r"^function %s\(" % fn, JL, flags=re.M), fn


def test_declared_set_equals_symbols_and_the_abi_version_stays_8():
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(dto_\w+)\(", H_NOCOMMENT, flags=re.M))
    assert declared == set(dto_amd.capi.SYMBOLS), declared ^ set(dto_amd.capi.SYMBOLS)
    assert not [n for n in declared if "tdb" in n]
    v = int(re.search(r"#define DTO_ABI_VERSION (\d+)", H).group(1))
    assert v == dto_amd.capi.DTO_ABI_VERSION == 8
    assert int(re.search(r"const DTO_ABI_VERSION = Int32\((\d+)\)", JL).group(1)) == 8


def test_the_entry_points_and_the_profile_names_are_documented():
    assert "Whole-dynamics solves" in H and '"dynsolve_couple"' in H and '"dynsolve_deriv"' in H
    for fn in (dto_amd.Evaluator.dynamics_layout, dto_amd.Evaluator.dynamics_solve_all, dto_amd.Evaluator.dynamics_solve_all_dev,
               dto_amd.Evaluator.feasible_trajectory, dto_amd.Evaluator.reduced_gradient):
        assert fn.__doc__


def test_a_structure_only_handle_answers_the_layout_and_refuses_the_solves():
    prob = three_level_problem(n=6, N=4)
    ev = dto_amd.Evaluator(to_engine(prob), device=-1)
    try:
        want = plan(describe(prob), prob.dt_idx, prob.N - 1)
        D, n_levels, offset, level = ev.dynamics_layout()
        assert (D, n_levels) == (want["n_states"], want["n_levels"]) == (16, 3)
        assert list(offset) == want["pre"] == [0, 6, 8, 14] and list(level) == want["level"] == [2, 1, 2, 0]
        lib = dto_amd.load_library()
        assert lib.dto_dynamics_layout(ev.handle, None, None, None, None) == 0     # every output is optional
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.dynamics_solve_all(prob.Z0, np.ones((4, 1, 16)))
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.dynamics_solve_all(prob.Z0, np.ones((4, 2, 16)), adjoint=True)
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.dynamics_solve_all_dev(0, 0, 1, 0)
        rows, cols = ev.jacobian_structure()   # the handle still answers
        assert rows.size == ev.n_jacobian_entries
        assert ev.dynamics_layout()[0] == 16
    finally:
        ev.close()


@pytest.mark.parametrize("name", list(REFUSED_LAYOUTS))
def test_the_three_plan_refusals_reach_the_caller_as_text(name):
    integs, z, text = REFUSED_LAYOUTS[name]
    h = RawDerivativeHandle(integs, z)
    try:
        assert text in h.layout()
        n_cons = C.c_int64()
        assert h.lib.dto_num_cons(h.h, C.byref(n_cons)) == 0 and n_cons.value == 3 * sum(d for _, d, _ in integs)   # still answers
    finally:
        h.close()


def test_the_layout_refuses_what_the_plan_refuses():
    p = O.make_external_integrator_problem()
    ev = dto_amd.Evaluator(to_engine(p), device=-1)
    try:
        with pytest.raises(dto_amd.EngineError, match="evaluated on the host"):
            ev.dynamics_layout()
        assert ev.integrator_share(0) == (0, 1, 0)
    finally:
        ev.close()
