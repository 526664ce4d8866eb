"""CPU: the Hessian-vector product entry points (dto_eval_hessian_product[_dev], MOI.eval_hessian_lagrangian_product) at the
boundary -- exported, typed alike in the header, ctypes and the Julia binding, and refused with text where no GPU evaluates."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import to_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = open(os.path.join(ROOT, "include", "dto_engine.h"), encoding="utf-8").read()
H_NOCOMMENT = re.sub(r"/\*.*?\*/", "", H, flags=re.S)
JL = open(os.path.join(ROOT, "integration", "DTOEngine.jl"), encoding="utf-8").read()
NAMES = ("dto_eval_hessian_product", "dto_eval_hessian_product_dev")
# C argument type -> the Julia type a @ccall must give it
JL_TYPE = {"dto_handle*": "Ptr{Cvoid}", "const double*": "Ptr{Float64}", "double*": "Ptr{Float64}", "double": "Float64",
           "void*": "Ptr{Cvoid}"}


def _prototype(name):
    m = re.search(r"^int\s+%s\((.*?)\);" % name, H_NOCOMMENT, flags=re.S | re.M)
    assert m, name
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    return [re.sub(r"\s+", " ", re.match(r"(.*?)(\w+)$", a).group(1).strip()).replace(" *", "*") for a in args]


def test_symbols_are_exported_and_the_abi_version_agrees():
    lib = dto_amd.capi.library_path()
    assert os.path.exists(lib), lib
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dto_\w+)$", out, flags=re.M))
    for n in NAMES:
        assert n in exported, n
        assert n in dto_amd.capi.SYMBOLS, n
    v = int(re.search(r"#define DTO_ABI_VERSION (\d+)", H).group(1))
    assert v == dto_amd.capi.DTO_ABI_VERSION == 8
    assert int(re.search(r"const DTO_ABI_VERSION = Int32\((\d+)\)", JL).group(1)) == v
    assert re.match(r"# DTOEngine\.jl .*ABI version %d\)" % v, JL.splitlines()[0]), JL.splitlines()[0]


def test_ctypes_prototypes_follow_the_header():
    ct = {"dto_handle*": dto_amd.capi.H, "const double*": (dto_amd.capi.c_double_p, C.c_void_p),
          "double*": (dto_amd.capi.c_double_p, C.c_void_p), "double": C.c_double, "void*": C.c_void_p}
    for n in NAMES:
        c_args = _prototype(n)
        res, py_args = dto_amd.capi.SYMBOLS[n]
        assert res is C.c_int and len(py_args) == len(c_args), (n, c_args, py_args)
        dev = n.endswith("_dev")
        for c, p in zip(c_args, py_args):
            want = ct[c]
            if isinstance(want, tuple):  # host form: double pointers; device form: opaque addresses
                want = want[1] if dev else want[0]
            assert p is want, (n, c, p)


def test_structure_only_handle_refuses_both_forms_with_text():
    ev = dto_amd.Evaluator(to_engine(O.make_readme_problem()), device=-1)
    try:
        Z = np.zeros(ev.n_variables)
        mu = np.zeros(ev.n_constraints)
        y = np.empty(ev.n_variables)
        with pytest.raises(dto_amd.EngineError, match="structure-only"):
            ev.eval_hessian_lagrangian_product(y, Z, np.ones(ev.n_variables), 1.0, mu)
        rc = ev._lib.dto_eval_hessian_product_dev(ev.handle, None, 1.0, None, None, None, None)
        assert rc != 0
        assert b"structure-only" in ev._lib.dto_last_error(ev.handle)
    finally:
        ev.close()


def test_julia_ccalls_have_the_header_signature():
    calls = re.findall(r"@ccall\(?\s*lib\.(dto_\w+)\((.*?)\)::(\w+)", JL, flags=re.S)
    seen = set()
    for name, args, ret in calls:
        if name not in NAMES:
            continue
        seen.add(name)
        assert ret == "Cint", name
        jl = [a.strip() for a in re.split(r",(?![^{]*\})", args) if a.strip()]
        c_args = _prototype(name)
        assert len(jl) == len(c_args), (name, jl, c_args)
        for a, c in zip(jl, c_args):
            assert a.split("::")[-1].strip() == JL_TYPE[c], (name, a, c)
    assert seen == set(NAMES), seen


def test_julia_shim_defines_the_moi_method_and_advertises_hessvec():
    m = re.search(r"^function MOI\.eval_hessian_lagrangian_product\(ev::GPUEvaluator, (\w+)::AbstractVector\{Float64\}, "
                  r"(\w+)::AbstractVector\{Float64\}, (\w+)::AbstractVector\{Float64\},\s*σ::Float64, μ::AbstractVector\{Float64\}\)",
                  JL, flags=re.M)
    assert m, "MOI.eval_hessian_lagrangian_product(ev, h, x, v, σ, μ) is not defined"
    body = JL[m.end():JL.index("\nend", m.end())]
    assert "stage_external!" in body and "dto_eval_hessian_product(" in body
    assert re.search(r"MOI\.features_available\(ev::GPUEvaluator\) = ev\.eval_hessian \? \[[^\]]*:HessVec[^\]]*\] : \[:Grad, :Jac\]", JL)
    assert "eval_hessian_lagrangian_product_dev!" in JL


def test_python_mirror_has_both_forms():
    assert callable(getattr(dto_amd.Evaluator, "eval_hessian_lagrangian_product", None))
    assert callable(getattr(dto_amd.Evaluator, "eval_hessian_product_dev", None))
