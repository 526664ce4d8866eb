"""CPU: dto_reduced_gradient / dto_reduced_hessian_product and their _dev forms at the boundary -- exported by the built library, typed
alike in the header, ctypes and the Julia binding, the header's declared set equal to capi.SYMBOLS, ABI version still 8, documented, and
a structure-only handle (no device) refuses all four with text and stays usable."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dto_amd
from elim_cases import three_level_problem
from helpers import to_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = open(os.path.join(ROOT, "include", "dto_engine.h"), encoding="utf-8").read()
H_NOCOMMENT = re.sub(r"/\*.*?\*/", "", H, flags=re.S)
JL = open(os.path.join(ROOT, "integration", "DTOEngine.jl"), encoding="utf-8").read()
NAMES = ("dto_reduced_gradient", "dto_reduced_gradient_dev", "dto_reduced_hessian_product", "dto_reduced_hessian_product_dev")

C_ARGS = {
    "dto_reduced_gradient": ["dto_handle* h", "const double* Z", "double sigma", "const double* mu", "double* grad", "double* lam"],
    "dto_reduced_gradient_dev": ["dto_handle* h", "const double* dZ", "double sigma", "const double* dmu", "double* dgrad", "double* dlam",
                                 "void* stream"],
    "dto_reduced_hessian_product": ["dto_handle* h", "const double* Z", "double sigma", "const double* mu", "const double* v", "double* y"],
    "dto_reduced_hessian_product_dev": ["dto_handle* h", "const double* dZ", "double sigma", "const double* dmu", "const double* dv",
                                        "double* dy", "void* stream"],
}


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
    H_, dp, vp = dto_amd.capi.H, dto_amd.capi.c_double_p, C.c_void_p
    host_ct, dev_ct = [H_, dp, C.c_double, dp, dp, dp], [H_, vp, C.c_double, vp, vp, vp, vp]
    host_jl = ["Ptr{Cvoid}", "Ptr{Float64}", "Float64", "Ptr{Float64}", "Ptr{Float64}", "Ptr{Float64}"]
    dev_jl = host_jl + ["Ptr{Cvoid}"]
    for name in NAMES:
        assert _c_args(name) == C_ARGS[name], name
        res, args = dto_amd.capi.SYMBOLS[name]
        assert res is C.c_int and list(args) == (dev_ct if name.endswith("_dev") else host_ct), name
        assert _jl_args(name) == (dev_jl if name.endswith("_dev") else host_jl), name
    for fn in ("reduced_gradient", "reduced_hessian_product", r"reduced_gradient_dev!", r"reduced_hessian_product_dev!"):
        assert re.search(r"^function %s\(" % fn, JL, flags=re.M), fn


def test_the_julia_host_wrappers_size_their_outputs_from_the_handle_and_check_lengths():
    """no caller-supplied size reaches the engine: the costates' first dimension is asked of dto_dynamics_layout, and Z, mu and v are
    checked against the problem's sizes before a pointer is taken"""
    grad = JL[JL.index("function reduced_gradient("):JL.index("function reduced_hessian_product(")]
    prod = JL[JL.index("function reduced_hessian_product("):JL.index("function reduced_gradient_dev!(")]
    assert "n_states" not in grad.split(")", 1)[0], "the size of the costates is no argument"
    assert "lib.dto_dynamics_layout(" in grad and "fill(NaN, Int(ns[]), ev.trajectory.N)" in grad
    assert 'reduced_check_lengths(ev, "reduced_gradient", Z, μ)' in grad and 'reduced_check_lengths(ev, "reduced_hessian_product", Z, μ, v)' in prod
    check = JL[JL.index("function reduced_check_lengths("):JL.index("function reduced_gradient(")]
    for size in ("length(Z) == ev.n_variables", "length(μ) == ev.n_constraints", "length(v) == ev.n_variables"):
        assert size in check, size


def test_declared_set_equals_symbols_and_the_abi_version_stays_8():
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(dto_\w+)\(", H_NOCOMMENT, flags=re.M))
    assert declared == set(dto_amd.capi.SYMBOLS), declared ^ set(dto_amd.capi.SYMBOLS)
    v = int(re.search(r"#define DTO_ABI_VERSION (\d+)", H).group(1))
    assert v == dto_amd.capi.DTO_ABI_VERSION == 8
    assert int(re.search(r"const DTO_ABI_VERSION = Int32\((\d+)\)", JL).group(1)) == 8


def test_the_entry_points_and_the_profile_name_are_documented():
    assert "Reduced-space operators" in H and '"reduced_pack"' in H
    for word in ("Cache rule", "Costs", "Workspaces", "Refused with text"):
        assert word in H[H.index("Reduced-space operators"):H.index("int dto_reduced_gradient(")], word
    for fn in (dto_amd.Evaluator.reduced_lagrangian_gradient, dto_amd.Evaluator.reduced_hessian_product,
               dto_amd.Evaluator.reduced_gradient_dev, dto_amd.Evaluator.reduced_hessian_product_dev):
        assert fn.__doc__


def test_a_structure_only_handle_refuses_all_four_with_text_and_stays_usable():
    prob = three_level_problem(n=6, N=4)
    ev = dto_amd.Evaluator(to_engine(prob), device=-1)
    try:
        v = np.ones(ev.n_variables)
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.reduced_lagrangian_gradient(prob.Z0)
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.reduced_lagrangian_gradient(prob.Z0, sigma=0.5, mu=np.ones(ev.n_constraints), costates=True)
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.reduced_hessian_product(prob.Z0, v)
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.reduced_gradient_dev(0, 1.0, 0, 0)
        with pytest.raises(dto_amd.EngineError, match="structure-only handle"):
            ev.reduced_hessian_product_dev(0, 1.0, 0, 0, 0)
        rows, cols = ev.jacobian_structure()   # the handle still answers
        assert rows.size == ev.n_jacobian_entries
        assert ev.dynamics_layout()[0] == 16
    finally:
        ev.close()
