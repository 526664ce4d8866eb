"""CPU: dto_dynamics_solve / dto_dynamics_solve_dev at the boundary -- exported by the built library, typed alike in the header, ctypes
and the Julia binding, the direction constants equal in all three, the header's declared set equal to capi.SYMBOLS, ABI version still
8, and a structure-only handle (no device) refuses the calls with text and stays usable."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import to_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = open(os.path.join(ROOT, "include", "dto_engine.h"), encoding="utf-8").read()
H_NOCOMMENT = re.sub(r"/\*.*?\*/", "", H, flags=re.S)
JL = open(os.path.join(ROOT, "integration", "DTOEngine.jl"), encoding="utf-8").read()

HOST_ARGS = ["dto_handle* h", "int32_t integrator", "const double* Z", "int32_t direction", "const double* B", "int32_t n_cols", "int32_t mode",
             "double* Y"]
DEV_ARGS = ["dto_handle* h", "int32_t integrator", "const double* dZ", "int32_t direction", "const double* dB", "int32_t n_cols", "int32_t mode",
            "double* dY", "void* stream"]


def _c_args(name):
    m = re.search(r"^int\s+%s\((.*?)\);" % name, H_NOCOMMENT, flags=re.S | re.M)
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def _jl_args(name):
    m = re.search(r"@ccall\(?\s*lib\.%s\((.*?)\)::(\w+)" % name, JL, flags=re.S)
    assert m and m.group(2) == "Cint", name
    return [a.split("::")[-1].strip() for a in re.split(r",(?![^{]*\})", m.group(1))]


def test_both_symbols_are_exported_by_the_built_library():
    lib = dto_amd.load_library()
    for name in ("dto_dynamics_solve", "dto_dynamics_solve_dev"):
        assert name in dto_amd.capi.SYMBOLS and hasattr(lib, name), name


def test_typed_alike_in_header_ctypes_and_julia():
    H_ = dto_amd.capi.H
    dp = dto_amd.capi.c_double_p
    assert _c_args("dto_dynamics_solve") == HOST_ARGS
    assert _c_args("dto_dynamics_solve_dev") == DEV_ARGS
    res, args = dto_amd.capi.SYMBOLS["dto_dynamics_solve"]
    assert res is C.c_int and list(args) == [H_, C.c_int32, dp, C.c_int32, dp, C.c_int32, C.c_int32, dp]
    res, args = dto_amd.capi.SYMBOLS["dto_dynamics_solve_dev"]
    assert res is C.c_int and list(args) == [H_, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    assert _jl_args("dto_dynamics_solve") == ["Ptr{Cvoid}", "Int32", "Ptr{Float64}", "Int32", "Ptr{Float64}", "Int32", "Int32", "Ptr{Float64}"]
    assert _jl_args("dto_dynamics_solve_dev") == ["Ptr{Cvoid}", "Int32", "Ptr{Float64}", "Int32", "Ptr{Float64}", "Int32", "Int32", "Ptr{Float64}",
                                                  "Ptr{Cvoid}"]
    assert re.search(r"^function dynamics_solve\(", JL, flags=re.M) and re.search(r"^function dynamics_solve_dev!\(", JL, flags=re.M)


def test_direction_constants_agree():
    defs = dict(re.findall(r"#define (DTO_SOLVE_\w+) (\d+)", H))
    assert defs == {"DTO_SOLVE_FORWARD": "0", "DTO_SOLVE_ADJOINT": "1"}
    assert (dto_amd.capi.SOLVE_FORWARD, dto_amd.capi.SOLVE_ADJOINT) == (0, 1)
    assert dict(re.findall(r"const (DTO_SOLVE_\w+) = Int32\((\d+)\)", JL)) == defs
    # the rollout's own set of constants is untouched
    assert dict(re.findall(r"#define (DTO_ROLLOUT_\w+) (\d+)", H)) == {"DTO_ROLLOUT_ALL": "0", "DTO_ROLLOUT_FINAL": "1"}


def test_declared_set_equals_symbols_and_the_abi_version_stays_8():
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(dto_\w+)\(", H_NOCOMMENT, flags=re.M))
    assert {"dto_dynamics_solve", "dto_dynamics_solve_dev"} <= declared
    assert declared == set(dto_amd.capi.SYMBOLS), declared ^ set(dto_amd.capi.SYMBOLS)
    assert not [n for n in declared if "tdb" in n]
    v = int(re.search(r"#define DTO_ABI_VERSION (\d+)", H).group(1))
    assert v == dto_amd.capi.DTO_ABI_VERSION == 8
    assert int(re.search(r"const DTO_ABI_VERSION = Int32\((\d+)\)", JL).group(1)) == 8


def test_the_entry_points_and_the_profile_names_are_documented():
    assert "Solves with the dynamics block" in H and all('"%s"' % n in H for n in ("dynsolve", "dynsolve_tree", "dynsolve_scan"))
    for f in (dto_amd.Evaluator.dynamics_solve, dto_amd.Evaluator.dynamics_solve_dev, dto_amd.Evaluator.rollout_gradient):
        assert f.__doc__ and "solve" in f.__doc__


def test_a_structure_only_handle_refuses_with_text_and_stays_usable():
    prob = O.make_scaled_problem(4, 5, 2, seed=1, skew=True)
    ev = dto_amd.Evaluator(to_engine(prob), device=-1)
    try:
        B = np.ones((4, 2, 5))
        for adjoint in (False, True):
            with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
                ev.dynamics_solve(prob.Z0, B, adjoint=adjoint)
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.dynamics_solve(prob.Z0, B, all_knots=False)
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.dynamics_solve_dev(0, 0, 1, 0)
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.rollout_gradient(prob.Z0, np.ones((4, 5)))
        rows, cols = ev.jacobian_structure()   # the handle still answers
        assert rows.size == ev.n_jacobian_entries
    finally:
        ev.close()
